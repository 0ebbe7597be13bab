/*
 * sybilgpu.h -- C ABI of the MI355X-native scan/aggregate engine for logv/sybil.
 *
 * This is the drop-in boundary for sybil's query hot path.  The reference has no
 * FFI/plugin interface; the seam this library replaces is the body of the per-block
 * loop in  src/lib/table_query.go:111-220  (LoadBlockFromDir -> CopyQuerySpec ->
 * FilterAndAggRecords -> block_specs[...]) together with the merge that follows
 * (MultiCombineResults/CombineResults, table_query.go:230-257,397-404 and
 * aggregate.go:361-467).  One call level up, the whole of
 *     count = t.LoadAndQueryRecords(&loadSpec, &querySpec)   (src/cmd/cmd_query.go:362)
 * maps to  sybl_query_prepare + sybl_query_scan (+ all-reduce) + sybl_query_finalize.
 * INTEGRATION.md shows the cgo shim a sybil maintainer would add.
 *
 * Conventions:
 *  - plain C types only; every entry point returns int (0 = ok, <0 = SYBL_E_*),
 *    sybl_last_error() gives the text for the calling thread; no exceptions or abort()
 *    cross the boundary.
 *  - the library never keeps a caller pointer after a call returns (cgo rule); inputs
 *    are consumed during the call, outputs live in library-owned memory until the
 *    matching *_free.
 *  - no globals: everything the reference reads from FLAGS/OPTS (config.go:119-120)
 *    is an explicit field of sybl_query_desc.
 *  - one sybl_ctx per GPU (one process per GPU under RCCL).  Thread-safe for concurrent
 *    calls from arbitrary OS threads (the reference queries blocks from 16 goroutines,
 *    table_query.go:110,230-231): calls on different ctx objects run concurrently; calls
 *    that take a handle of ONE ctx -- the ctx, its tables, queries and results -- are
 *    serialised by the library (a per-ctx lock held for the length of each call), so a
 *    thread may read a result's rows while another scans or frees the query behind it.
 *    What stays the caller's business is ORDER, not exclusion: a handle must not be used
 *    after its *_free, and scan -> [allreduce] -> [snapshot] -> finalize of one query are
 *    issued in that order.
 *  - there is NO CPU fallback: without a usable HIP device every compute call fails
 *    with SYBL_E_NODEVICE.
 */
#ifndef SYBILGPU_H
#define SYBILGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYBL_ABI_VERSION 6

enum {
    SYBL_OK = 0,
    SYBL_E_INVAL = -1,    /* bad argument / unknown column / unsupported query shape */
    SYBL_E_NODEVICE = -2, /* no HIP device, or a HIP call failed */
    SYBL_E_NOMEM = -3,
    SYBL_E_IO = -4,       /* table directory / gob decode problem */
    SYBL_E_STATE = -5,    /* call order violated (e.g. finalize before scan) */
    SYBL_E_BLOCK = -6     /* a block was rejected (the reference skips such blocks) */
};

/* record.go:14-19 */
enum { SYBL_NO_VAL = 0, SYBL_INT_VAL = 1, SYBL_STR_VAL = 2, SYBL_SET_VAL = 3 };

/* filter ops: filter.go:176-190 (int), :213-245 (str), :268-283 (set) */
enum {
    SYBL_OP_GT = 0, SYBL_OP_LT = 1, SYBL_OP_EQ = 2, SYBL_OP_NEQ = 3,
    SYBL_OP_RE = 4, SYBL_OP_NRE = 5, SYBL_OP_IN = 6, SYBL_OP_NIN = 7
};

/* FLAGS.OP (aggregate.go:24-29) */
enum { SYBL_AGG_AVG = 0, SYBL_AGG_HIST = 1 };

#define SYBL_MAX_GROUPS 8
#define SYBL_MAX_AGGS 6
#define SYBL_MAX_FILTERS 16
#define SYBL_GROUP_BY_WIDTH 8 /* aggregate.go:16 */
#define SYBL_BLOCK_ROWS 65536 /* table.go:44 CHUNK_SIZE */

typedef struct sybl_ctx sybl_ctx;
typedef struct sybl_table sybl_table;
typedef struct sybl_query sybl_query;
typedef struct sybl_result sybl_result;

/* ------------------------------------------------------------------ context */

int sybl_abi_version(void);
/* Text of the last error raised on the calling thread ("" if none). */
const char *sybl_last_error(void);

/* device: HIP device ordinal of this process' GPU (LOCAL_RANK under torchrun). */
int sybl_init(int device, sybl_ctx **out);
void sybl_shutdown(sybl_ctx *ctx);
/* Run all work of this ctx on an existing hipStream_t (e.g. the host framework's
 * current stream); NULL restores the ctx's own stream. */
int sybl_ctx_set_stream(sybl_ctx *ctx, void *hip_stream);
int sybl_ctx_sync(sybl_ctx *ctx);
/* Gives back what the ctx keeps between calls for speed and a long-running host may not want to pay for: the loader's
 * staging arena (up to ~512 MB of pinned host memory and as much HBM, kept from one sybl_table_open / sybl_table_refresh to
 * the next because pinning it costs every load tens of milliseconds).  A host that opens its tables once and then only
 * queries them calls this after the last open; the next load allocates the arena again.  ABI 4. */
int sybl_ctx_trim(sybl_ctx *ctx);
int sybl_device_info(sybl_ctx *ctx, char *name, size_t name_cap, int *n_cus, int64_t *hbm_bytes);

/* ------------------------------------------------------------------ tables
 * A table is the HBM-resident form of a sybil table: one dense array per column
 * (reference value types: IntField int64, StrField int32 dictionary id, SetField
 * []int32 -- record_fields.go:8-10), a validity bitmap for columns with missing
 * rows, and a table-global string dictionary per str/set column (the reference's
 * are block-local, table_column.go:27-48; SURVEY.md 8a note 8).                  */

int sybl_table_create(sybl_ctx *ctx, const char *name, sybl_table **out);
void sybl_table_free(sybl_table *t);

/* Declare a column before the first block is appended.  info_min/info_max are the
 * table-level IntInfo.Min/Max (table_column_info.go:18-24, loaded from info.db by
 * the host) that hist geometry and the outlier gate use (aggregate.go:254,
 * hist_basic.go:104).  Pass min > max to let the library use the exact extrema. */
int sybl_table_add_column(sybl_table *t, const char *name, int type, int64_t info_min, int64_t info_max);

/* One host-decoded column of one block (what unpackIntCol/unpackStrCol/unpackSetCol
 * produce, column_store_io.go:493-780), handed over columnar. */
typedef struct {
    const char *name;
    int32_t type;             /* SYBL_INT_VAL | SYBL_STR_VAL | SYBL_SET_VAL */
    const int64_t *ints;      /* INT: nrows values */
    const int32_t *str_ids;   /* STR: nrows ids into `strings` (block-local dictionary) */
    const int64_t *set_off;   /* SET: nrows+1 CSR offsets */
    const int32_t *set_ids;   /* SET: member ids into `strings` */
    const uint8_t *populated; /* nrows bytes 0/1 (Record.Populated != _NO_VAL); NULL = all rows */
    const char *const *strings; /* STR/SET: block StringTable */
    int32_t n_strings;
} sybl_col_view;

/* Appends one block (<= 65536 rows in the reference, any size here).  Columns of the
 * table that are absent from `cols` are unpopulated for the whole block. */
int sybl_table_append_block(sybl_table *t, int64_t nrows, int32_t ncols, const sybl_col_view *cols);

/* Device-side deterministic generator for benchmarks and parity tests (SURVEY.md 8d;
 * the formula is restated in oracle/sybil_oracle.c:orc_synth_fill).  Every column is a
 * fully populated INT column. */
enum { SYBL_SYN_UNIFORM = 0, SYBL_SYN_TIME = 1, SYBL_SYN_BELL = 2 };
typedef struct {
    const char *name;
    int32_t kind;      /* SYBL_SYN_* */
    int32_t col_index; /* salt of the per-column hash stream */
    int64_t a, b;      /* UNIFORM: [a, a+b)   TIME: a + floor(i*b/N)   BELL: a + 4 x [0,b) */
    int64_t info_min, info_max; /* IntInfo given to hists; min > max = exact extrema */
} sybl_synth_col;
/* Rows [row0, row0+nrows) of a virtual table of total_rows rows (a rank's shard). */
int sybl_table_create_synth(sybl_ctx *ctx, const char *name, uint64_t seed, int64_t total_rows,
                            int64_t row0, int64_t nrows, int32_t ncols, const sybl_synth_col *cols,
                            sybl_table **out);

/* Native loader: reads a sybil table directory written by the reference
 * (<dir>/<table>/info.db and <block>/{info.db,int_*.db,str_*.db,set_*.db}[.gz],
 * table_io.go:132, table_block_io.go:225-310) straight into HBM.  `columns` limits
 * the load to the referenced columns like LoadSpec does (table_load_spec.go:59-73);
 * NULL loads every column.  rank/nranks shard the block list contiguously. */
int sybl_table_open(sybl_ctx *ctx, const char *dir, const char *table, const char *const *columns,
                    int32_t n_columns, int32_t rank, int32_t nranks, sybl_table **out);

/* sybl_table_open with options.  SYBL_OPEN_COMPACT: the table is in compact storage from the first
 * block on (each decoded block is packed into place, columns widen when a block needs it), so a table
 * whose canonical form would not fit in HBM can still be loaded. */
#define SYBL_OPEN_COMPACT 1
int sybl_table_open_flags(sybl_ctx *ctx, const char *dir, const char *table, const char *const *columns,
                          int32_t n_columns, int32_t rank, int32_t nranks, int32_t flags, sybl_table **out);

/* Writes the resident table under <dir>/<table name>/ in the reference's on-disk format (block
 * directories with info.db + int_/str_/set_<col>.db gob files, table info.db: column_store_io.go:64-358,
 * table_io.go:40-78) -- bucket encoded at <= 5000 distinct values per block, else value encoded -- so a
 * `sybil` binary or sybl_table_open can read it back. */
int sybl_table_save(sybl_table *t, const char *dir);

/* Test hook (no GPU needed): the gob bytes sybl_table_save writes for one block of an INT column (kind
 * SYBL_INT_VAL) or a STR column (SYBL_STR_VAL; vals = ids into dict).  Library-owned, valid until the next call
 * on the thread. */
const void *sybl_debug_encode_column(int kind, const char *name, const int64_t *vals, const uint8_t *populated, int64_t n,
                                     const char *const *dict, int64_t n_dict, int64_t *n_bytes);

/* Where the time of the last sybl_table_open of this table went (disk -> HBM, the "TableBlock load" half of the hot
 * path).  Worker threads read and gob-decode column files a window of blocks ahead; the calling thread interns
 * dictionaries, copies the compact decoded pieces through a pinned ring and launches the decode kernels in block
 * order. */
typedef struct {
    double wall_s;          /* sybl_table_open, start to finish */
    double parse_cpu_s;     /* CPU time (CLOCK_THREAD_CPUTIME_ID) summed over worker threads: file read + gob decode + flatten */
    double wait_s;          /* calling thread blocked on the next block's worker */
    double apply_s;         /* calling thread: dictionaries, pinned-ring copies, kernel launches, block commit */
    int64_t file_bytes;     /* bytes read from column / info files (after gunzip) */
    int64_t h2d_bytes;      /* bytes that crossed PCIe */
    int32_t workers, blocks;
    /* SYBL_LOADER_GPU_VARINT=1 (ABI 5): column files whose varints were walked on the GPU (csrc/gobgpu.hip), and blocks the
     * host parser then loaded again because a walk reported damage or values outside the block's info.db bounds */
    int32_t gpu_varint_cols, gpu_varint_redone;
} sybl_load_stats;
int sybl_table_load_stats(const sybl_table *t, sybl_load_stats *out);

/* Makes a table opened with sybl_table_open* follow its directory: block directories that appeared since are loaded
 * behind the resident ones, blocks that vanished leave the scan, blocks whose <block>/info.db changed (digest rewrote
 * them) are dropped and loaded again, and the columns' IntInfo is re-read from the table's info.db.  The resident
 * table replaces the reference's per-query re-listing of the directory (table_query.go:40-106) and its per-block
 * result cache (query_cache.go:30-64); this call is what keeps it current.  Prepared queries must be prepared again
 * (SYBL_E_STATE otherwise).  Any of the counters may be NULL.  Dropped rows stay in HBM, unreferenced, until the table
 * is reopened. */
int sybl_table_refresh(sybl_table *t, int64_t *n_added, int64_t *n_dropped, int64_t *n_reloaded);

/* Blocks sybl_table_open skipped the way the reference does: unreadable block info.db, NumRecords
 * <= 0, or a column file whose record ids / value count exceed NumRecords ("BLOCK SIZE CHANGED
 * DURING QUERY", column_store_io.go:524-526,572-574,733-735; table_query.go:134-139). */
int64_t sybl_table_broken_blocks(const sybl_table *t);

int64_t sybl_table_rows(const sybl_table *t);
int64_t sybl_table_blocks(const sybl_table *t);
int64_t sybl_table_hbm_bytes(const sybl_table *t);
/* Exact extrema of an INT column over resident rows and the IntInfo in force. */
int sybl_table_column_info(const sybl_table *t, const char *name, int *type, int64_t *exact_min,
                           int64_t *exact_max, int64_t *info_min, int64_t *info_max, int *has_missing);
/* Multi-rank hosts: declare bounds that hold on EVERY rank (all-reduce the exact extrema
 * first) so that the direct-mapped group layout, and therefore the partial tables, are
 * identical across ranks.  has_missing != 0 reserves the MISSING_VALUE key slot.  lo > hi (no rank holds a
 * value) declares no bounds but still applies has_missing. */
int sybl_table_set_bounds(sybl_table *t, const char *name, int64_t lo, int64_t hi, int has_missing);
/* Group-by on a key column whose value RANGE is too wide for direct mapping (more than 2^22
 * values, or more than 2^27 cells together with the other keys) goes through a dictionary of the
 * column's DISTINCT values (at most 2^22), built on the GPU on first use.  Multi-rank hosts make
 * the dictionaries identical: gather sybl_table_column_distinct from every rank, install the
 * union with sybl_table_set_group_dict on every rank.  `values` is library-owned (valid until the
 * column changes). */
int sybl_table_column_distinct(sybl_table *t, const char *name, const int64_t **values, int64_t *n);
int sybl_table_set_group_dict(sybl_table *t, const char *name, const int64_t *values, int64_t n);
/* Str / set dictionaries (table-global ids are assigned in first-seen order per process).  Ranks of
 * a multi-GPU job gather every rank's dictionary and install the same union everywhere; resident
 * ids are remapped in place.  The new dictionary must contain every resident value. */
int sybl_table_column_dict(sybl_table *t, const char *name, const char *const **strings, int64_t *n);
int sybl_table_set_dict(sybl_table *t, const char *name, const char *const *strings, int64_t n);
/* Compact storage.  Canonical device storage mirrors the reference's Record fields: int64 per INT
 * value (IntField, record_fields.go:8), int32 per STR id (StrField).  sybl_table_compact re-encodes
 * every INT / STR column as unsigned offsets from the column's exact minimum at the narrowest of
 * 1, 2, 4 bytes that holds max - min (8 when it does not fit) -- the in-HBM counterpart of the
 * reference's bucket / delta encoded column files (column_store_io.go:64-358).  Every kernel decodes
 * while loading, so query results are identical; a scan streams the compact bytes.  The table stays
 * in compact mode: blocks appended later are packed into place (a column is re-encoded wider when a
 * block does not fit its width / base; call compact again to re-narrow).  On an empty table the call
 * only switches the mode on.  Installing a str dictionary returns that column to int32 ids.
 * Prepared queries must be prepared again afterwards (SYBL_E_STATE otherwise). */
int sybl_table_compact(sybl_table *t);
/* bytes per stored value and the value base of a column as currently laid out in HBM */
int sybl_table_column_storage(const sybl_table *t, const char *name, int32_t *width, int64_t *base);
/* Copies rows [row0,row0+n) of an INT column back to the host (tests, samples). */
int sybl_table_read_int(const sybl_table *t, const char *name, int64_t row0, int64_t n, int64_t *out);

/* ------------------------------------------------------------------ queries
 * sybl_query_desc mirrors QueryParams (query_spec.go:25-41) plus the FLAGS/OPTS the
 * hot loop reads (aggregate.go:100, hist_basic.go:79,111, hist.go:29-31).         */

typedef struct {
    const char *col;
    int32_t op;            /* SYBL_OP_* ; the column's type selects Int/Str/SetFilter */
    int64_t int_value;     /* IntFilter.Value */
    const char *str_value; /* StrFilter/SetFilter.Value (literal, or regex for RE/NRE) */
    /* optional: RE/NRE evaluated by the host per dictionary entry (Go's regexp), one
     * byte per table-global id; overrides str_value when non-NULL */
    const uint8_t *id_match;
    int64_t id_match_len;
} sybl_filter;

/* -str-replace col:pattern:replacement (table_query.go:33-46, column_store_io.go:517-545): when a block is unpacked, every
 * string of the column's StringTable is rewritten with regexp.ReplaceAllString and strings that become equal share one
 * id -- so str filters compare, and group-by groups, the REWRITTEN strings.  Here the dictionaries are resident and
 * table-global: the rewrite is a property of the query.  Either `pattern` + `replace` (the library's RE2 engine,
 * $1 / ${name} / $$ expanded as regexp.Expand does) or, when `replaced` is non-NULL, the host's own result: one
 * rewritten string per table-global dictionary id (sybl_table_column_dict order).  Only str columns are rewritten. */
typedef struct {
    const char *col;
    const char *pattern;
    const char *replace;
    const char *const *replaced;
    int64_t n_replaced;
} sybl_str_replace;

typedef struct {
    int32_t n_filters;
    const sybl_filter *filters; /* ANDed (aggregate.go:105-116) */
    int32_t n_groups;
    const char *const *groups;  /* int or str columns (set group-by is rejected, cmd_query.go:254) */
    int32_t n_aggs;
    const char *const *aggs;    /* int columns */
    int32_t op;                 /* SYBL_AGG_AVG | SYBL_AGG_HIST */
    int64_t hist_bucket;        /* FLAGS.HIST_BUCKET, 0 = auto */
    /* HIST only: 1 = keep every bucket array (percentiles and buckets can be output);
     * 0 = moments only: count/sum/avg/min/max and the reference's bucket-quantised
     * stddev are produced from four exact integer accumulators. */
    int32_t want_percentiles;
    const char *time_col;       /* with time_bucket > 0: time-series query */
    int64_t time_bucket;        /* QuerySpec.TimeBucket */
    const char *weight_col;     /* OPTS.WEIGHT_COL.  Weights below 1 are not supported: the reference indexes out of range once a
                                 * running count turns negative, and the bounds that recover avg and stddev assume Count > 0 */
    const char *order_by;       /* "$COUNT", an aggregated column, or NULL/"" = unsorted */
    int32_t order_asc;
    int32_t limit;              /* FLAGS.LIMIT; <= 0 = all groups */
    int32_t block_skip;         /* ShouldLoadBlockFromDir min/max pruning (table_block_io.go:110-182) */
    /* FLAGS.LOG_HIST (-loghist): MultiHist instead of BasicHist (hist.go:27-38, hist_multi.go) -- with op HIST a chain
     * of sub-histograms whose ranges halve from Info.Max downwards; percentiles and stddev come from the union of their
     * buckets.  Bucket arrays are always kept (want_percentiles is implied); sybl_result_subhists describes them. */
    int32_t loghist;
    int32_t n_str_replace;              /* QueryParams.StrReplace (query_spec.go:30) */
    const sybl_str_replace *str_replace;
    /* -distinct (QuerySpec.Distincts, query_spec.go:29; aggregate.go:205-243): every Result also keeps a count-distinct
     * sketch of the listed columns' combined value; sybl_result_distinct reads it and the renderers print it where the
     * reference prints Distinct.Cardinality() (printer.go:79-80,142-144,204-205).  Either int columns (at most
     * SYBL_MAX_GROUPS; the reference's fast path) or exactly one str column (its slow path over one column); a list
     * mixing str with other columns is refused (SYBL_E_INVAL).  The sketch is the reference's dependency
     * github.com/logv/loglogbeta restated from the published algorithms (PARITY UNPINNED: DESIGN.md section 7). */
    int32_t n_distincts;
    const char *const *distincts;
    /* ABI 4.  1 = the caller is a PRINTER (printSortedResults / printResults / -json: printer.go:25-308): of Results it looks
     * at the first `limit` rows of the sort order and at Cumulative, as the reference does -- GetPercentiles / GetStdDev are
     * print-time calls there (printer.go:60-76), made for the rows that are printed.  With limit > 0, op HIST, bucket arrays
     * kept and 2048 group cells or more, percentiles / stddev / bucket arrays are then produced for those rows and
     * Cumulative only: the other rows of sybl_result_rows carry count / samples / sum / avg / min / max, percentiles = NULL,
     * values = NULL and stddev = NaN.  What it saves: the summary pass over every group's bucket array per query (config 4:
     * 0.28 ms and 52 MB of percentiles per step) and, across ranks, the reduce-scatter of the whole bucket table -- only the
     * cell fields, Cumulative's buckets and the printed rows' arrays travel (~1 MB instead of 263 MB per rank;
     * sybl_query_collective_finalize is then 1: snapshot and finalize are collective).  0 (the default, and what
     * -encode-results needs: every Result travels whole, printer.go:263-289): every row carries everything.
     * 2 (ABI 5): as 1, and the rows beyond `limit` need nothing but their Count -- what both printers of the reference look at
     * (printer.go:154-158: sorted[:Limit]).  When the order is $COUNT descending the limit is then pushed INTO the scan
     * (csrc/pushdown.hip): group counts from the key column alone, the printed groups chosen on the device, one pass over key
     * and value columns for Cumulative and those groups -- no bucket array exists for any other group.  Taken for a single
     * direct-mapped key of at most 65 536 cells without filters (sybl_run_stats.strategy = 8); any other query answers as
     * with 1.  The rows beyond the limit then report sum 0 / avg 0 / min, max at their initial values.
     * Across ranks (sybl_comm_init): sybl_query_scan of such a query is a COLLECTIVE call -- at the first scan the ranks ask
     * each other whether every one of them planned the pushed-down scan (a rank without rows cannot; then none takes it), and
     * every pushed-down scan all-reduces the groups' counts between its two passes so that all ranks print the same groups.
     * (A host that merges the ranks' partial tables with collectives of its own -- sybl_query_partials -- must pass 0 or 1: the
     * library cannot make its ranks agree on the printed groups.) */
    int32_t printed_only;
} sybl_query_desc;

int sybl_query_prepare(sybl_table *t, const sybl_query_desc *desc, sybl_query **out);
void sybl_query_free(sybl_query *q);

/* Launches the scan of this rank's resident rows on the ctx stream; asynchronous. */
int sybl_query_scan(sybl_query *q);

/* The rank-local partial group table, laid out identically on every rank of a job:
 * `sum` words combine with SUM, `max` words with MAX (minima are stored as their bitwise
 * complement ~v since ABI 6: like -v it reverses the order, and it has no overflow at INT64_MIN).
 * Multi-GPU hosts all-reduce both buffers in place (RCCL over xGMI) between
 * sybl_query_scan and sybl_query_finalize; single-GPU hosts skip this. */
int sybl_query_partials(sybl_query *q, void **d_sum, int64_t *n_sum_words, void **d_max, int64_t *n_max_words);
/* Optional: make the scan write its partials into caller-owned device buffers
 * (e.g. torch tensors) of at least the sizes sybl_query_partials reports. */
int sybl_query_bind_partials(sybl_query *q, void *d_sum, void *d_max);

/* In-library RCCL path for hosts without a collective runtime of their own (the Go
 * host): unique_id is the 128-byte ncclUniqueId produced by sybl_comm_unique_id on
 * rank 0 and distributed by the host. */
int sybl_comm_unique_id(void *id128);
int sybl_comm_init(sybl_ctx *ctx, const void *id128, int32_t nranks, int32_t rank);
int sybl_comm_free(sybl_ctx *ctx);
/* COLLECTIVE (every rank, same order).  The first call on a query also compares the ranks' partial-table layouts and
 * fails with SYBL_E_STATE on EVERY rank when they differ (bounds or dictionaries were not agreed: sybl_table_agree) --
 * instead of summing unrelated words or hanging.  Collectives hold the ctx's lock while they wait for the other ranks. */
int sybl_query_allreduce(sybl_query *q);
/* rank / number of ranks of the ctx's communicator (0 / 1 without one).  ABI 5. */
int sybl_comm_info(const sybl_ctx *ctx, int32_t *rank, int32_t *nranks);
/* COLLECTIVE over the ctx's communicator (sybl_comm_init), called by every rank once its shard of the table is resident
 * (sybl_table_open with rank / nranks, or appended blocks) and again after a sybl_table_refresh that loaded blocks: the
 * whole agreement a multi-GPU job needs before its partial tables line up, so that a host without a collective runtime
 * of its own -- the Go host -- runs N ranks through this library alone.  (1) the ranks must hold the same columns
 * (SYBL_E_STATE on every rank otherwise); (2) INT columns: bounds = the extrema over ALL ranks' rows (one MAX all-reduce,
 * minima complemented), has_missing = any rank's -- what sybl_table_set_bounds declares by hand; (3) STR / SET columns:
 * every rank installs the SORTED union of the ranks' dictionaries (sybl_table_set_dict; resident ids renumbered in place)
 * and the union of has_missing; (4) for each int column of `group_cols` (the columns the host is about to group by, in
 * -group order; NULL / 0 = none) whose agreed range the planner would group through a dictionary of distinct values: the
 * union of the ranks' distinct values becomes every rank's dictionary (sybl_table_set_group_dict); when some rank -- or the
 * union -- holds more values than a dictionary may, every rank's planner takes the hash table instead.  Without a
 * communicator (one GPU) the call only sorts the str / set dictionaries, so that the order of equal-count groups in the
 * output does not depend on how many GPUs ran the query.  Prepared queries must be prepared again.  Replaces the
 * reference's key translation at merge time (aggregate.go:284-324,414-467; node_aggregator.go:147-177).  ABI 5. */
int sybl_table_agree(sybl_table *t, const char *const *group_cols, int32_t n_group_cols);

/* Hash group-by (group keys that do not direct-map: more than 2^27 possible cells, or a key column with more than 2^22
 * distinct values -- the reference's map[string]*Result, aggregate.go:186-200).  The scan aggregates into an
 * open-addressing table; afterwards the partial table is the DENSE, key-ordered list of the groups this rank found, so
 * its size is only known after the scan (sybl_query_partials then reports it; sybl_query_bind_partials is refused).
 * sybl_query_allreduce runs the whole multi-rank protocol.  Hosts with their own collective runtime do it in three
 * steps: gather every rank's sybl_query_hash_keys (ascending 62-bit composite keys; n = 0 and keys = NULL for a
 * direct-mapped query), install the sorted union on every rank with sybl_query_hash_install_union (the partial tables
 * then have identical layouts), all-reduce the buffers sybl_query_partials returns.  `keys` is library-owned, valid
 * until the next scan / union install of the query. */
int sybl_query_hash_keys(sybl_query *q, const uint64_t **keys, int64_t *n);
int sybl_query_hash_install_union(sybl_query *q, const uint64_t *keys, int64_t n);

/* 1 when the last sybl_query_allreduce left part of the merge to the finalize: big histogram tables with a row limit
 * are either reduce-SCATTERED (every rank keeps the reduced arrays of a slice of the cells, derives its percentiles there
 * and the summaries are all-gathered) or, for a printer (sybl_query_desc.printed_only), not sent at all -- the ranks
 * all-reduce the cell fields, derive the same sort order, and sum Cumulative's buckets and the printed rows' arrays
 * only.  sybl_query_snapshot and sybl_query_finalize are then COLLECTIVE: every rank calls them, in the same order;
 * every rank gets the full result.  0: rank-local calls as usual. */
int sybl_query_collective_finalize(const sybl_query *q);

/* Optional: enqueue the device -> host copy of the (reduced) partials now (after the all-reduce on
 * multi-GPU hosts).  A following sybl_query_finalize then waits for that copy only, not for work
 * enqueued behind it -- a host serving a stream of queries overlaps the finalize of one query with
 * the scan of the next (two prepared queries, alternating). */
int sybl_query_snapshot(sybl_query *q);
/* Copies the (reduced) partials to the host (unless sybl_query_snapshot already did), finds the groups that exist and
 * sorts them (SortResults, aggregate.go:497-525).  Waits for the copy (hence for the scan and the all-reduce before
 * it).  The ROWS of a result with 2048 groups or more -- avg / stddev / percentiles, GroupByKey strings, the
 * sybl_group_row array -- are built when first asked for (sybl_result_rows, sybl_result_render, sybl_result_encode),
 * from the result's own reference-counted snapshot: the reference's Results are its accumulators (aggregate.go:186-203),
 * nothing has to be built before a printer walks them, and a time series of 360 000 rows or a 65 536-group histogram
 * costs the step that finalizes it nothing it does not print.  The query may be scanned again in between.  A result
 * whose rows carry keys of their own (hash group-by, key spaces beyond 2^18 cells) builds them from the query's group
 * columns and the table's dictionaries: it stays registered with its query, and sybl_query_free builds the rows of
 * such results that are still alive before the query goes away (the table must outlive its queries, as always). */
int sybl_query_finalize(sybl_query *q, sybl_result **out);

/* ------------------------------------------------------------------ results */

typedef struct {
    int32_t present;      /* 0: this group never saw an INT value for the aggregation */
    int64_t count;        /* BasicHist.Count (weighted) */
    int64_t samples;      /* BasicHist.Samples */
    int64_t sum;          /* the LOW 64 BITS of the exact  sum(v*w)  over accepted values (a group of 5 400 microsecond
                           * timestamps already leaves int64) */
    double avg;           /* true sum/count (reference: running mean, <=1e-6 rel).  The true sum is recovered from `sum`, the
                           * count n and the bounds [lo, hi] of the accepted values while n*(hi - lo) < 2^64 (the group's own
                           * extrema where they are tracked, then (n-2)*(hi - lo); else the column's); beyond that -- four rows
                           * of 9e18 next to one of -4e18 -- avg, stddev and the printed sum come from the wrapped sum */
    double stddev;        /* GetStdDev semantics (hist_basic.go:192-219); 0 in AVG mode.  Where it comes from the bucket moments
                           * sb = sum(b*w) and sb2 = sum(b*b*w) (no percentiles wanted, or 2048+ groups), each kept mod 2^64, the true
                           * sb2 is recovered from its low bits, sb and Count while (n_values-1)*sb - sb*sb/Count < 2^64 (always
                           * when (n_values-1)^2 * Count < 2^64: any Count below 1.8e13); beyond that stddev comes from the wrapped sb2 */
    int64_t min, max;     /* BasicHist.Min/Max incl. the reference's initial values */
    int64_t bucket_size;  /* HIST: BasicHist.BucketSize */
    int64_t num_buckets;  /* HIST: BasicHist.NumBuckets */
    int64_t n_values;     /* HIST: len(Values) */
    const int64_t *values;      /* HIST + want_percentiles: bucket counts, else NULL */
    const int64_t *percentiles; /* HIST + want_percentiles: 100 entries (GetPercentiles), else NULL */
    int64_t n_outliers;   /* accepted values clipped into an edge bucket (BasicHist.Outliers + Underliers, all blocks) */
    /* HIST + want_percentiles: the outliers' values (ascending; those below hist Min are the reference's Underliers),
     * as the reference remembers them (hist_basic.go:132-142) and prints them as buckets of their own (:239-257).
     * n_outlier_values = -1: not available -- the query's outlier log overflowed (SYBL_OUTLIER_LOG_CAP, default 2^20
     * values per query) or the result was merged across ranks (the values stay on the rank that saw them); the
     * renderers then refuse -json / -encode-results for rows with outliers instead of printing wrong buckets.
     * The reference itself keeps only ONE block's list per histogram after merging (BasicHist.Combine does not merge
     * them, hist_basic.go:259-279) and none in Cumulative: this is the deterministic superset. */
    const int64_t *outlier_values;
    int64_t n_outlier_values;
} sybl_agg_out;

typedef struct {
    const uint8_t *binary_key; /* Result.BinaryByKey: 8 LE bytes per group column */
    const char *group_by_key;  /* Result.GroupByKey: values joined and terminated by '\t' */
    int64_t time_bucket;       /* TimeResults key (0 for all-time results) */
    int64_t count;             /* Result.Count */
    int64_t samples;           /* Result.Samples */
    const sybl_agg_out *aggs;  /* n_aggs entries */
} sybl_group_row;

/* -loghist results: how the `values` array of aggregation `agg` is laid out.  Sub-histogram k (Subhists[k] of the
 * reference's MultiHist, hist_multi.go:223-257) owns values[offset .. offset + n_values): its BasicHist.Values; and
 * values[ext_offset .. ext_offset + n_ext): one exact counter per value from ext_first upwards -- how often that value
 * was an Outlier of the sub-histogram (beyond its last bucket: clipped into it AND remembered, hist_basic.go:132-135;
 * counted per occurrence, not per weight).  sybl_agg_out.bucket_size / num_buckets are 0 for such rows and
 * n_outliers is the sum of the ext counters.  The array is library-owned (valid until the result is freed); n = 0
 * for a query without loghist. */
typedef struct {
    int64_t info_min, info_max;   /* the sub-histogram's Info range (inclusive) */
    int64_t bucket_size, num_buckets, n_values;
    int64_t offset;               /* of its Values inside sybl_agg_out.values */
    int64_t ext_first, n_ext, ext_offset;
} sybl_subhist;
int sybl_result_subhists(const sybl_result *r, int agg, const sybl_subhist **subs, int64_t *n);

/* (the first call on a lazily finalized result builds its rows: see sybl_query_finalize)
 * which: 0 = Results (every group, sorted by order_by; the limit is applied when rendering,
 *            as printSortedResults does), 1 = TimeResults (by bucket, then key),
 *        2 = Cumulative ("TOTAL", one row) */
int sybl_result_rows(const sybl_result *r, int which, const sybl_group_row **rows, int64_t *n);
int64_t sybl_result_matched(const sybl_result *r); /* QuerySpec.MatchedCount */

/* Count-distinct queries (sybl_query_desc.distincts): Result.Distinct of row `row` of sybl_result_rows(which) --
 * *cardinality = Distinct.Cardinality(); *registers (may be NULL) = the sketch's SYBL_HLL_REGISTERS bytes, library-owned
 * until the result is freed (a host that merges results of several nodes takes the register-wise maximum,
 * query_spec.go:180-188).  SYBL_E_INVAL for a query without distincts or a row out of range. */
#define SYBL_HLL_REGISTERS 16384
int sybl_result_distinct(const sybl_result *r, int which, int64_t row, int64_t *cardinality, const uint8_t **registers);
void sybl_result_free(sybl_result *r);

typedef struct {
    int64_t rows_scanned;     /* rows of blocks that were not skipped */
    int64_t blocks_scanned, blocks_skipped;
    int64_t algorithmic_bytes;/* rows_scanned x sum of stored widths of referenced columns (as laid out in HBM) */
    int64_t canonical_bytes;  /* the same with canonical widths (8 per INT value, 4 per STR id) */
    double scan_ms;           /* hipEvent time of the scan kernel(s) of the last sybl_query_scan */
    double reduce_ms;         /* partial-table fold kernels */
    int32_t n_cells;          /* direct-mapped group cells */
    int32_t strategy;         /* 0 = LDS cell table (generic kernel), 1 = global atomics, 2 = LDS cell table
                               * (role-specialised kernel), 3 / 4 = per-workgroup LDS time window (generic /
                               * role-specialised kernel), 5 = partitioned histograms, 6 = cell table AND
                               * bucket arrays in LDS, 7 = hash group-by (open-addressing table in HBM behind an
                               * LDS staging table; n_cells = slots of the table), 8 = -limit pushed into the scan of a
                               * printer's histogram query (printed_only = 2; csrc/pushdown.hip) */
    int32_t lds_bytes, n_workgroups, replicas;
    int32_t n_sum_fields;     /* int64 fields per cell in the SUM section */
    int32_t n_max_fields;     /* fields per cell in the MAX section; 0 = nothing to MAX-reduce */
    int32_t packed_kernel;    /* 1: the scan ran k_scan_packed (compact storage, 32-bit offset domain) */
    int32_t count_pass_reused;/* strategy 5: 1 = the last scan reused the per-(workgroup, bin) record counts its query's first scan
                               * took (they depend on the table's rows, the filters and the key columns only) and skipped the
                               * counting pass over the key column.  ABI 5. */
} sybl_run_stats;
/* Valid after the stream has been synchronised (sybl_query_finalize / sybl_ctx_sync). */
int sybl_query_stats(sybl_query *q, sybl_run_stats *out);

/* Test hook: the exact integer accumulators behind the last finalized result, by direct-mapped cell
 * (cell = time-bucket index x group cells + sum of (key - min) x stride, first group column most
 * significant): which = 0 Count, 1 sum(v), 2 sum(b), 3 sum(b^2) of aggregation `agg` (b = the reference's
 * bucket index, hist_basic.go:130; 2 and 3 exist in moments mode and when percentiles were summarised on
 * the GPU).  Writes min(cap, n_cells) values; *n_cells = cells of the query.  Full-size parity tests compare
 * these with the CPU oracle bit for bit. */
int sybl_debug_query_cells(sybl_query *q, int which, int agg, int64_t *out, int64_t cap, int64_t *n_cells);

/* reference output surface (printer.go:109-232,291-308): renders a result the way
 * `sybil query` prints it.  format: 0 = text table, 1 = -json.  Returns a
 * library-owned NUL-terminated buffer valid until the result is freed. */
const char *sybl_result_render(sybl_result *r, int format);

/* `-encode-results` (printer.go:284-289): the result as encoding/gob of NodeResults{QuerySpec{QueryParams,
 * QueryResults{Cumulative, Results, TimeResults, MatchedCount, Sorted}}} with HistCompat histograms --
 * what `sybil aggregate` (node_aggregator.go) and src/api consume.  Library-owned buffer valid until the
 * result is freed; bucket arrays are included for the rows that carry them. */
const void *sybl_result_encode(sybl_result *r, int64_t *n_bytes);

/* ------------------------------------------------------------------ samples
 * `sybil query -samples` (cmd_query.go:330-343, table_query.go:96-228, printer.go:388-476): the ROWS behind a filter,
 * newest first or ordered by an int column.  Filters are the aggregate path's (ANDed, strict, an unpopulated row fails);
 * matching rows are selected and their values gathered on the GPU (csrc/samples.hip).
 *
 * The reference visits blocks one at a time and stops after the first block at which the matched count so far is STRICTLY
 * greater than -limit, concatenates the visited blocks' Matched lists in Go map order (random), reverses or sorts, and
 * truncates.  Restated deterministically, with block order for the map order (one of the orders the reference can produce):
 *   blocks b = 0..B-1 in resident order; m_b = rows of block b that pass every filter;
 *   blocks_visited P = the smallest p >= 1 with m_0 + .. + m_(p-1) > limit, or B if there is none;
 *   candidates c_0 < c_1 < .. < c_(M-1) = the matching rows of blocks 0..P-1 in ascending row order; matched = M;
 *   L = min(limit, M).
 *   order_by NULL, "" or "$COUNT" (order_asc is ignored, as in the reference): c_(M-1), c_(M-2), .. -- the first L.
 *   order_by = an INT column k: D = the candidates ordered by: rows without k first, then value descending; equal values,
 *     and the rows without k among themselves, by descending row.  order_asc = 0: the first L of D; order_asc = 1: the
 *     first L of D reversed (the reference reverses, then truncates).
 *   order_by = a STR or SET column: SYBL_E_INVAL (the reference would compare block-local ids, record.go:60-73).
 *   limit = 0: no rows; limit < 0: SYBL_E_INVAL; a table without blocks: no rows.
 * Filters on more than 8 distinct columns are refused (SYBL_E_INVAL).
 * Out of scope: -str-replace on samples; -encode-results of samples (gob interface{} values); the text form (PrintRecord
 * prints a Go pointer dump); multi-rank merging -- the calls are rank-local and never collective, a host concatenates and
 * truncates the ranks' rows as node_aggregator.go:59-79 does. */
typedef struct {
    int32_t n_filters;
    const sybl_filter *filters;  /* as in sybl_query_desc */
    int32_t n_columns;
    const char *const *columns;  /* columns to return; NULL / 0 = every column (LoadAllColumns) */
    const char *order_by;        /* NULL, "", "$COUNT", or an int column */
    int32_t order_asc;
    int32_t limit;               /* FLAGS.LIMIT; >= 0 */
} sybl_samples_desc;

typedef struct sybl_samples sybl_samples;

/* Runs on the ctx stream and is complete on return.  The result owns everything it shows, strings included: it stays valid
 * after sybl_table_free. */
int sybl_table_samples(sybl_table *t, const sybl_samples_desc *d, sybl_samples **out);
void sybl_samples_free(sybl_samples *s);

typedef struct {
    int64_t n_rows;          /* output rows (L) */
    int64_t matched;         /* M */
    int64_t blocks_visited;  /* P */
    int64_t blocks_total;    /* B */
    int64_t blocks_filtered; /* blocks the filter pass ran over (the visit proceeds in windows of blocks; 0 without filters) */
    int32_t n_columns;
    double filter_ms;        /* hipEvent time of the filter passes */
    double select_ms;        /* hipEvent time of count, prefix, compaction, sort and gather */
} sybl_samples_info;
int sybl_samples_get_info(const sybl_samples *s, sybl_samples_info *out);

/* One returned column over the n_rows output rows.  Only the arrays of the column's type are non-NULL. */
typedef struct {
    const char *name;
    int32_t type;                    /* SYBL_INT_VAL | SYBL_STR_VAL | SYBL_SET_VAL */
    const uint8_t *populated;        /* n_rows bytes 0/1 */
    const int64_t *ints;             /* INT: n_rows values (0 where unpopulated) */
    const int32_t *str_ids;          /* STR: the table-global dictionary ids (-1 where unpopulated) */
    const char *const *strings;      /* STR: strings[i] = row i's string, NULL where unpopulated */
    const int64_t *set_off;          /* SET: n_rows + 1 CSR offsets over the output rows */
    const char *const *set_strings;  /* SET: the members' strings in stored order */
} sybl_samples_col;
int sybl_samples_column(const sybl_samples *s, int32_t i, sybl_samples_col *out);
/* The table-wide logical row index of every output row (row 0 = the first row of the first block). */
int sybl_samples_row_ids(const sybl_samples *s, const int64_t **logical_rows);
/* -json: printJson([]*Sample) -- what encoding/json makes of the rows: "[]" when empty, else per row an object whose keys
 * are the populated columns' names in bytewise sorted order; ints as decimals, strings escaped as encoding/json does (HTML
 * escaping included), sets as arrays of strings.  Library-owned, valid until the result is freed. */
const char *sybl_samples_render(sybl_samples *s);

/* ------------------------------------------------------------------ digest
 * The reference's write path sorts the records by Timestamp before it cuts them into blocks (SaveRecordsToColumns,
 * table_io.go:119-130; saveRecordList, table_io.go:80-117; Timestamp = the time column's value, Go's zero for a row without
 * one: column_store.go:9-20, column_store_io.go:741-743,768-770).  sybl_table_digest is that step for a resident table: the
 * table's rows in time order, cut into blocks, as a NEW resident table.  Key extraction, the sort and the gather of every
 * column run on the GPU (csrc/digest.hip).  Restated deterministically:
 *   source rows: the logical rows of the live blocks in resident order, r = 0..N-1.  Blocks without rows (left behind by
 *     sybl_table_refresh) and the padding between blocks contribute nothing.
 *   key k(r) = the value of time_col in row r if it is populated, else 0; keys compare as signed int64.
 *   order: ascending k, STABLE -- equal keys keep source order.  (sort.Sort in the reference is unstable; the stable order is
 *     one of the orders it can produce, and the one defined here.)
 *   time_col: NULL or "" = "time" (the default of FLAGS.TIME_COL).  A name the table does not hold, or a column that is not
 *     an INT column: SYBL_E_INVAL.  (The reference would sort on all-zero keys for an unknown name; this call refuses.)
 *   block_rows: 0 = 65536 (CHUNK_SIZE, table.go:44); 1..65536 as given; anything else: SYBL_E_INVAL.
 *   output block j holds sorted rows [j * block_rows, min(N, (j+1) * block_rows)).  N = 0: the columns and no blocks.
 * The output table: same ctx, same name, the same columns in the same order with their type and IntInfo; the str / set
 * dictionaries copied id for id (an id means the same string in both tables); declared bounds (sybl_table_set_bounds) and
 * has_missing copied; compact storage iff the source is in compact mode (every output value is a source value: the source
 * columns' widths and bases are kept).  It is not attached to a directory.  Group dictionaries and derived columns are not
 * copied: the next prepare builds them as for any table.  Per-block min / max / populated counts are exact for the new
 * blocks; table-wide extrema may be the source's (bounds of a superset are bounds).
 * The source table is untouched and its version does not move: prepared queries on it stay valid.  The output owns
 * everything it shows and outlives the source; free it with sybl_table_free.
 * Rank-local, never collective; runs on the ctx stream and is complete on return.  N >= 2^31 rows: SYBL_E_INVAL (the sort
 * counts its items in an int); so are more than 2^32 - 1 physical rows in the source, dead blocks included (source rows
 * travel as 32-bit numbers).  The call needs the table's size again plus, per row, two keys (4 bytes each when the
 * time column's range -- with 0 in it, if a row lacks the column -- fits 32 bits, else 8), two 4-byte row numbers and the sort's scratch; when
 * HBM runs out it returns SYBL_E_NOMEM, frees everything it allocated and leaves *out NULL. */
int sybl_table_digest(sybl_table *t, const char *time_col, int32_t block_rows, sybl_table **out);

/* Where the device time of the sybl_table_digest that made this table went (zeros for any other table), and the bytes each
 * phase moves, computed from the shapes. */
typedef struct {
    int64_t rows, blocks;  /* N, output blocks */
    int32_t key_bits;      /* bits of the key the sort ordered by */
    double keys_ms;        /* hipEvent time: key extraction */
    double sort_ms;        /* ... the radix sort */
    double gather_ms;      /* ... gather of every column, validity words and block statistics */
    int64_t keys_bytes, sort_bytes, gather_bytes;
} sybl_digest_stats;
int sybl_table_digest_stats(const sybl_table *t, sybl_digest_stats *out);

/* ------------------------------------------------------------------ select
 * The rows of a resident table that pass a filter, as a NEW resident table: what keeps a subset of a table in HBM.  Its uses:
 * retention for resident tables (select time > T, free the old table -- the reference trims whole blocks, table_trim.go);
 * materialising an expensive filter once, so that the queries behind it are plain scans of a smaller table; and, followed by
 * sybl_table_save, the export of a subset in the reference's format (-export, table_query.go:204).  The filter pass, the row
 * list and the gather of every column run on the GPU (csrc/select.hip).  Restated deterministically:
 *   source rows: the logical rows of the live blocks in resident order, r = 0..N-1.  Blocks without rows (left behind by
 *     sybl_table_refresh) and the padding of a block to 32 rows contribute nothing.
 *   matching: a row matches when it passes every filter, evaluated exactly as the aggregate path and samples do: ANDed,
 *     strict, an unpopulated value fails.  Without filters every row matches (the call then re-cuts the table into other
 *     block sizes).  When the planner proves that no row can match (x > INT64_MAX, an operator the column's type does not
 *     have) the output has the columns and no blocks, and no kernel runs; filters it does not see through (x > 5 AND x < 3)
 *     run the kernels, find M = 0 and give the same output.  Filters on more than 8 distinct columns: SYBL_E_INVAL (as
 *     for samples).
 *   output rows: the matching rows in ascending source order, s_0 < s_1 < .. < s_(M-1).  Output block j holds
 *     s_[j * block_rows, min(M, (j+1) * block_rows)).  M = 0: the columns and no blocks.
 *   block_rows: 0 = 65536; 1..65536 as given; anything else: SYBL_E_INVAL.
 *   columns: the output holds the named columns in the order named, each once (a name given again is ignored); NULL or 0 =
 *     every column in table order; a name the table does not hold: SYBL_E_INVAL.  A filter column need not be an output column.
 * Every output column inherits, by digest's rules: type, IntInfo, declared bounds (sybl_table_set_bounds) and has_missing;
 * the str / set dictionary copied id for id; compact storage iff the source is in compact mode, with the source column's
 * (width, base) kept (every output value is a source value); a validity bitmap iff the source column has one.  Per-block
 * min / max / populated counts are exact for the new blocks; table-wide extrema may be the source's.
 * The output has the source's ctx and name, is attached to no directory, owns everything it shows and outlives the source;
 * free it with sybl_table_free.  The source is untouched and its version does not move: prepared queries on it stay valid.
 * Rank-local, never collective; runs on the ctx stream and is complete on return.  More than 2^32 - 1 physical rows in the
 * source, dead blocks included: SYBL_E_INVAL (row numbers travel as 32 bits; nothing is sorted, so no 2^31 limit applies).
 * The call needs a bit per source row, 4 bytes per matching row and the output; when HBM runs out it returns SYBL_E_NOMEM,
 * frees everything it allocated and leaves *out NULL.  NULL arguments are errors. */
typedef struct {
    int32_t n_filters;
    const sybl_filter *filters;   /* as in sybl_query_desc / sybl_samples_desc */
    int32_t n_columns;
    const char *const *columns;   /* columns of the output; NULL / 0 = every column */
    int32_t block_rows;           /* 0 = 65536; 1..65536 as given */
} sybl_select_desc;

int sybl_table_select(sybl_table *t, const sybl_select_desc *d, sybl_table **out);

/* Where the device time of the sybl_table_select that made this table went (zeros for any other table), and the bytes each
 * phase moves, computed from the shapes. */
typedef struct {
    int64_t rows_in, rows_out, blocks_in, blocks_out;  /* N, M, live source blocks, output blocks */
    double filter_ms;      /* hipEvent time: bitmap memset + k_prefilter (0 without filters) */
    double rows_ms;        /* ... k_sel_count + k_sel_rows (the readback between them is not in it) */
    double gather_ms;      /* ... gather of every output column, validity words and block statistics */
    int64_t filter_bytes, rows_bytes, gather_bytes;
} sybl_select_stats;
int sybl_table_select_stats(const sybl_table *t, sybl_select_stats *out);

/* ------------------------------------------------------------------ concat
 * Resident tables joined end to end as a NEW resident table: the call that takes more than one table.  Its uses: folding a
 * small table of arrivals into a big digested one (digest the arrivals, concat, free both: a streaming copy, not a sort of
 * everything); one table out of tables kept per day or per shard; putting two selects back together.  The reference has no
 * such call: the semantics are this library's.  Dictionaries are table-global and compact storage is per table, so the
 * rows are RE-ENCODED where the stored forms differ; that runs on the GPU (csrc/concat.hip).  Restated deterministically:
 *   source rows: for each source in the order given, the logical rows of its live blocks in resident order.  Blocks without
 *     rows (left behind by sybl_table_refresh) and the padding of a block to 32 rows contribute nothing.  A table may
 *     appear more than once; one table alone gives a copy of it.
 *   blocks: block boundaries are KEPT -- the output's blocks are the sources' live non-empty blocks in that order, output
 *     block k starting at the next multiple of 32 physical rows.  Nothing is re-cut (sybl_table_select without filters
 *     does that) and nothing is sorted (sybl_table_digest does that).  Zero rows in total: the columns and no blocks, and
 *     no kernel runs.
 *   columns: NULL or 0 = the union of the sources' columns in first-seen order (source 0's columns in its order, then each
 *     later source's new ones); otherwise the named columns in the order named, each once (a name given again is
 *     ignored).  A name that no source holds: SYBL_E_INVAL.  The same name with different types in two sources:
 *     SYBL_E_INVAL, the message names the column and both tables.  A source that lacks an output column contributes
 *     unpopulated rows for its blocks.
 *   dictionaries (str / set): the output dictionary is the first holder's (source 0's, when it holds the column) id for id,
 *     then, for each later source in order, that source's strings in its id order where the output does not hold them yet.
 *     Every source's WHOLE dictionary takes part, used by a row or not.  So the first holder's ids are unchanged and the
 *     others go through one id -> id table per (source, column); a later source whose table is the identity needs none.
 *   storage: the output is in compact mode iff EVERY source is.  In compact mode each int / str column is stored, as
 *     sybl_table_compact stores it, at the narrowest of 1 / 2 / 4 / 8 bytes that holds hi - lo, as offsets from base lo
 *     (the canonical width -- 8 for ints, 4 for str ids -- has base 0).  For an int column [lo, hi] is the union of the
 *     tracked extrema (sybl_table_column_info: exact_min, exact_max) of the sources that hold it; for a str column the
 *     union, over the sources, of the tracked id extrema [a, b] -- for a source with an id table T, of min and max of
 *     T[a..b].  A column with no populated row anywhere: width 1, base 0.  Otherwise canonical: int64 values, int32 ids,
 *     base 0.  sybl_table_column_storage reports it.
 *   validity: an output column has a bitmap iff some source column has one, or some source with rows lacks the column.
 *     Padding bits are zero.
 *   inherited: the type; IntInfo -- given iff every source holding the column was given one, then the minimum of the minima
 *     and the maximum of the maxima, otherwise the exact extrema are in force as for info_min > info_max; has_missing --
 *     the OR over the sources, or true when a source with rows lacks the column.  NOT inherited: declared bounds
 *     (sybl_table_set_bounds speaks of another table's ranks), group dictionaries, rank columns, carried weights: the next
 *     prepare builds them.
 *   statistics: per-block min / max / populated counts and the table-wide extrema are exact or the sources' own (bounds of
 *     a superset are bounds); those of a str column whose ids went through an id table are recomputed.
 * The output has source 0's ctx and name, is attached to no directory, owns everything it shows and outlives every source;
 * free it with sybl_table_free.  The sources are untouched and their versions do not move: a query prepared on a source
 * before the call still scans afterwards.  Sources of different contexts, n_tables < 1, a NULL entry, NULL d or out:
 * SYBL_E_INVAL, sybl_last_error begins "sybl_table_concat: ".  When HBM runs out: SYBL_E_NOMEM, everything freed, *out NULL.
 * Rank-local, never collective; runs on the ctx stream, is complete on return and thread-safe per ctx like select.  There
 * is no 2^31 or 2^32 row limit: nothing is sorted and no row numbers travel.  A table with set columns pays a host pass
 * per set column (their CSR is concatenated on the host). */
typedef struct {
    int32_t n_tables;
    sybl_table *const *tables;     /* >= 1, same ctx; a table may appear more than once */
    int32_t n_columns;
    const char *const *columns;    /* columns of the output; NULL / 0 = the union of the sources' columns */
} sybl_concat_desc;

int sybl_table_concat(const sybl_concat_desc *d, sybl_table **out);

/* What the sybl_table_concat that made this table did (zeros for any other table).  A piece is one (source, int / str
 * output column) pair of a source with rows that holds the column. */
typedef struct {
    int64_t rows, blocks;    /* of the output */
    int32_t tables, columns; /* sources given, output columns */
    int32_t copies;          /* pieces in the output's stored form: device-to-device copies */
    int32_t transcodes;      /* pieces re-encoded at another width / base (k_cc_transcode) */
    int32_t lut_transcodes;  /* ... and through an id table */
    int32_t runs;            /* runs of consecutive live blocks, over all sources */
    double copy_ms;          /* hipEvent time of all device copies, transcodes and validity words */
    double stats_ms;         /* ... of the recomputed block statistics */
    int64_t copy_bytes;      /* bytes copy_ms moved (read + written), computed from the shapes */
} sybl_concat_stats;
int sybl_table_concat_stats(const sybl_table *t, sybl_concat_stats *out);

/* ------------------------------------------------------------------ lookup
 * Columns of a second resident table attached by key, as a NEW resident table: what adds a column that comes from somewhere
 * else.  A table is an event log of ids (user, host, build); what the ids mean lives in a small second table `dim` (host to
 * datacenter, build to release date).  For every row of t the call finds the row of dim whose key equals the row's key and
 * attaches chosen columns of that dim row: a LEFT JOIN with FIRST MATCH, in broadcast form -- every rank holds all of dim.
 * The reference has no join: the semantics are this library's.  Key table, probe and gather run on the GPU (csrc/lookup.hip);
 * everything behind the call is a plain scan of a resident table.  Restated deterministically:
 *   rows and blocks: exactly what sybl_table_concat of t alone gives -- t's live non-empty blocks in resident order, block
 *     boundaries kept, each block starting on a multiple of 32 physical rows; dead blocks and padding contribute nothing.
 *     The columns of t come out as that concat gives them: values, dictionaries, storage, validity, statistics, and the list
 *     of what is not inherited.  t without rows: all the columns (attached ones included), no blocks, and no kernel runs.
 *   keys: `key` names the key column of t, `dim_key` that of dim (NULL or "" = the name given in key).  Both are INT columns
 *     or both are STR columns; a SET key, two key types, or a name the table does not hold: SYBL_E_INVAL, the message names
 *     the column.  INT keys compare as decoded int64 values -- the stored width and base may differ between the tables.  STR
 *     keys compare as strings, not ids: the two dictionaries are unrelated.  A row of t whose key is unpopulated matches
 *     nothing; rows of dim whose key is unpopulated take no part.
 *   which dim row: among the live dim rows with a populated key equal to the row's key, the FIRST in resident order.  The
 *     later ones are counted (sybl_lookup_stats.dim_duplicates).  dim without rows: nothing matches.
 *   attached columns: `columns` names the dim columns to attach, in the order named, each once (a name given again is
 *     ignored); NULL or 0 = every dim column except dim_key, in dim's order.  dim_key itself may be attached when it is
 *     named.  A name dim lacks: SYBL_E_INVAL.  An attached column is named prefix + name (prefix NULL = ""); a name the
 *     output already holds -- a column of t, or an earlier attached one --: SYBL_E_INVAL naming it.  For output row r with
 *     match m the value is dim's value at row m; it is populated iff there is a match and dim's value at m is populated;
 *     where it is unpopulated the stored bytes are 0.  An attached column inherits the dim column's type, IntInfo and
 *     dictionary id for id.  Declared bounds (sybl_table_set_bounds) are NOT inherited, as in concat.  has_missing is dim's
 *     OR "some row of t found no match".  It has a validity bitmap iff the dim column has one or some row found no match;
 *     padding bits are zero.
 *   storage: the output is in compact mode iff t is.  In compact mode each attached int / str column is stored at the
 *     narrowest of 1 / 2 / 4 / 8 bytes that holds the dim column's tracked extrema (for a str column: of its ids), as
 *     offsets from the minimum -- concat's rule; a column with no populated row: width 1, base 0.  Otherwise canonical: int64
 *     values, int32 ids, base 0.  The stored form of a dim column and of its output column can differ: the gather re-encodes.
 *   set columns of dim may be attached; as in digest and concat their CSR is built on the host, from the match list.
 *   statistics: per-block min / max / populated counts of the attached columns are exact; table-wide extrema may be dim's
 *     (bounds of a superset are bounds).
 * dim may hold at most 2^32 - 2 physical rows (the all-ones row number means "no match"); beyond: SYBL_E_INVAL.  An INT key
 * whose values are too spread for a direct table goes through a hash table of at most kHashMaxSlots = 2^27 slots; a dim that
 * needs more: SYBL_E_INVAL, the message says so.  t has no row limit.  When HBM runs out: SYBL_E_NOMEM, everything freed,
 * *out NULL.  NULL t, d, out or d->dim, a dim of another context, a negative n_columns: SYBL_E_INVAL; sybl_last_error begins
 * "sybl_table_lookup: ".
 * Both sources are untouched and their versions do not move: a query prepared on either before the call still scans
 * afterwards.  dim may be t itself.  The output has t's ctx and name, is attached to no directory, owns everything it shows
 * and outlives both sources; free it with sybl_table_free.  Rank-local, never collective; runs on the ctx stream, is complete
 * on return and thread-safe per ctx like select.
 * Out of scope: inner joins (follow with sybl_table_select on an attached column); many-to-many expansion (one dim row per
 * row of t, the first); composite keys; a CLI flag; any distribution of dim across ranks. */
typedef struct {
    sybl_table *dim;              /* same ctx as t; may be t itself */
    const char *key;              /* key column of t */
    const char *dim_key;          /* key column of dim; NULL or "" = the name given in key */
    int32_t n_columns;
    const char *const *columns;   /* dim columns to attach; NULL / 0 = every dim column except dim_key, in dim's order */
    const char *prefix;           /* put before each attached column's name; NULL = "" */
} sybl_lookup_desc;

int sybl_table_lookup(sybl_table *t, const sybl_lookup_desc *d, sybl_table **out);

/* What the sybl_table_lookup that made this table did (zeros for any other table): the device time of its phases and the
 * bytes each moves, computed from the shapes. */
typedef struct {
    int64_t rows, blocks;                         /* of the output */
    int64_t dim_rows, dim_keys, dim_duplicates;   /* live dim rows; distinct populated keys; populated dim rows - dim_keys */
    int64_t matched;                              /* rows of t that found a dim row */
    int64_t slots;                                /* hash path: slots of the table, else 0 */
    int32_t path;          /* 1 = direct over the key's range, 2 = hash, 3 = str ids; 0 = no key table was built (t or dim
                              without rows, no populated dim key) */
    int32_t columns;       /* attached */
    double build_ms, probe_ms, gather_ms;             /* hipEvent time: key table; probe; gather, validity, block statistics */
    int64_t build_bytes, probe_bytes, gather_bytes;
} sybl_lookup_stats;
int sybl_table_lookup_stats(const sybl_table *t, sybl_lookup_stats *out);

/* ------------------------------------------------------------------ compute
 * INT columns computed from expressions over a table's columns, as a NEW resident table: the projection that makes a new value
 * (latency = end - start, is_error = status >= 500, hour = time % 86400 / 3600, coalesce(region_id, 0)).  Queries group, filter
 * and aggregate over stored columns only; this call stores the value once, at the narrowest width that holds its ACTUAL range,
 * and everything behind it is a plain scan of a resident table.  The reference has no such call: the semantics are this
 * library's.  Evaluation, extrema and storage run on the GPU (csrc/compute.hip).  Restated deterministically:
 *   rows, blocks and the columns of t: exactly what sybl_table_concat of t alone gives -- t's live non-empty blocks in resident
 *     order, block boundaries kept, each block starting on a multiple of 32 physical rows; the columns of t come out as that
 *     concat gives them (values, dictionaries, storage, validity, statistics, and the list of what is not inherited).  The
 *     computed columns follow t's columns in the order given.  Expression k is evaluated on the OUTPUT's columns row by row, so it
 *     may name computed columns 0 .. k-1.  t without rows: all the columns (computed ones included), no blocks, no kernel runs.
 *   expressions: the result is always an INT column.
 *     literals: decimal digits, value <= 2^63; 9223372036854775808 wraps to INT64_MIN so that -9223372036854775808 can be written.
 *     columns: a name [A-Za-z_][A-Za-z0-9_]*, or any name between backticks; a name followed by ( is a function.  A column read
 *       as a value must be an INT column of the output; STR and SET columns may appear only as the argument of has().
 *     operators, C precedence, the binary ones left-associative: unary - !   * / %   + -   < <= > >=   == !=   &&   ||   and
 *       parentheses.  Functions: min(a,b) max(a,b) abs(a) if(c,a,b) coalesce(a,b) has(col).
 *     values: signed 64-bit integers with Go's semantics.  + - * unary - and abs wrap mod 2^64; / truncates toward zero; % takes
 *       the dividend's sign; INT64_MIN / -1 == INT64_MIN and INT64_MIN % -1 == 0.  Comparisons, ! && || give 1 or 0; truth is
 *       != 0.
 *     populated or not: a column operand is unpopulated where its validity bit is clear.  An operator or function with an
 *       unpopulated operand gives an unpopulated result -- && and || included: both sides are always evaluated, nothing
 *       short-circuits.  / and % by a populated zero give an unpopulated result (Go would panic; this call does not).
 *       if(c,a,b) is unpopulated where c is; elsewhere it takes the value AND the populatedness of the chosen branch only (a zero
 *       divisor in the other branch does not matter).  coalesce(a,b) is a where a is populated, else b with b's populatedness.
 *       has(col) is 1 or 0, always populated: for any column type the bit sybl_samples_column reports as `populated`.
 *     limits, each SYBL_E_INVAL: more than 8 distinct columns per expression (the filters' limit), more than 64 postfix ops, an
 *       operand stack deeper than 8, parentheses or calls nested deeper than 64.
 *     not in the language: bit operators and shifts, string-valued expressions, set membership, anything floating point.
 *   each computed column: type INT; no IntInfo (the exact extrema are in force); no dictionary; no declared bounds.  It is
 *     populated exactly where the expression is; the stored bytes are 0 where it is unpopulated and in padding rows.  has_missing
 *     is true iff some live row is unpopulated, and it has a validity bitmap iff some live row is unpopulated (padding bits zero).
 *   storage: compact iff the output is in compact mode (iff t is).  In compact mode the column is stored at the narrowest of
 *     1 / 2 / 4 / 8 bytes that holds hi - lo, as offsets from lo, over the EXACT minimum lo and maximum hi of the populated
 *     results -- concat's rule; with no populated row: width 1, base 0.  Otherwise canonical int64, base 0.
 *   statistics: per-block min / max / populated counts and the table-wide extrema are exact.
 * SYBL_E_INVAL, sybl_last_error beginning "sybl_table_compute: " and naming the expression's column (for syntax errors with the
 * byte offset): NULL t, d, out, exprs, a NULL name or expr; n_exprs < 1; an empty name; a name the output already holds (a column
 * of t or an earlier computed one); an unknown column; a STR or SET column used as a value; a syntax error; a wrong argument
 * count; a literal above 2^63; any of the limits.  Everything that can be refused is refused before anything is made; *out is
 * NULL after any failure.  When HBM runs out: SYBL_E_NOMEM, everything freed.
 * t is untouched and its version does not move: a query prepared on it before the call still scans afterwards.  The output has
 * t's ctx and name, is attached to no directory, owns everything it shows and outlives t; free it with sybl_table_free.
 * Rank-local, never collective; runs on the ctx stream, is complete on return and thread-safe per ctx like select.  There is no
 * row limit: no row numbers travel.
 * Out of scope: a CLI flag; fusing an expression into a query's scan; STR or SET results; float results; aggregates or window
 * functions inside expressions. */
typedef struct {
    const char *name;   /* of the computed column */
    const char *expr;
} sybl_compute_col;
typedef struct {
    int32_t n_exprs;
    const sybl_compute_col *exprs;
} sybl_compute_desc;

int sybl_table_compute(sybl_table *t, const sybl_compute_desc *d, sybl_table **out);

/* What the sybl_table_compute that made this table did (zeros for any other table). */
typedef struct {
    int64_t rows, blocks;        /* of the output */
    int32_t exprs, ops;          /* expressions; sum of their program lengths */
    int64_t unpopulated;         /* sum over the expressions of the live rows whose result is unpopulated */
    double range_ms, store_ms, stats_ms;   /* hipEvent time: extrema passes; store passes + validity; block statistics */
    int64_t range_bytes, store_bytes;      /* computed from the shapes */
} sybl_compute_stats;
int sybl_table_compute_stats(const sybl_table *t, sybl_compute_stats *out);

/* Test hooks (no GPU needed) for compute expressions: the host build of the parser and of the very op functions the kernel uses
 * (csrc/compute_expr.h, csrc/compute_ops.h).  names / types: the n_cols columns the expression may name (types[i]: SYBL_INT_VAL /
 * SYBL_STR_VAL / SYBL_SET_VAL).  sybl_debug_compute_program: the postfix form, e.g. "c0 c1 sub 1000 div" -- c<k> is the k-th
 * distinct column of the expression, has(c<k>) its populated bit, constants by value, ops by name; NULL (and sybl_last_error) on
 * a refusal.  Library-owned buffer, valid until the next call on the thread.  sybl_debug_compute_eval: values / populated are
 * [n_cols][n_rows]; out / out_populated get n_rows results (0 where unpopulated). */
const char *sybl_debug_compute_program(const char *expr, int32_t n_cols, const char *const *names, const int32_t *types);
int sybl_debug_compute_eval(const char *expr, int32_t n_cols, const char *const *names, const int32_t *types, const int64_t *values,
                            const uint8_t *populated, int64_t n_rows, int64_t *out, uint8_t *out_populated);

/* ------------------------------------------------------------------ rollup
 * A group-by whose result is again a resident table: one row per group, aggregated on the GPU (csrc/rollup.hip), which the
 * engine can scan, save, concat, look up and roll up like any other table -- pre-aggregation (an hourly rollup by host kept
 * resident while the raw table is freed), two-level aggregation (a histogram over a per-user count), a materialised group-by
 * as the small side of sybl_table_lookup.  The reference has no such call; the semantics are this library's.  Restated
 * deterministically:
 *   source rows: the logical rows of t's live blocks in resident order, N of them; dead blocks and padding contribute nothing.
 *   matching: every filter is evaluated exactly as sybl_table_select evaluates it (ANDed, strict, an unpopulated value fails,
 *     at most 8 distinct filter columns).  When the planner proves that nothing matches the output is the columns and no
 *     blocks, and no kernel runs.  A filter column need not be a key or an aggregated column.
 *   key: an optional time part, then the n_groups (0..4) group columns in the order named.  Group columns are INT or STR; a SET
 *     column, an unknown name, a name given twice or more than 4 columns: SYBL_E_INVAL naming it.  time_bucket > 0 makes
 *     time_col (NULL / "" = "time"; an INT column) part of the key: the bucket value is v / B * B with Go's truncating division
 *     (aggregate.go:174, the key of the reference's TimeResults), so -1 and 1 both fall into bucket 0; a matching row whose
 *     time column is unpopulated is dropped and counted (rows_no_time), as the reference's time series does.  time_bucket = 0:
 *     no time part; time_bucket < 0: SYBL_E_INVAL.  An unpopulated group value is a group of its own (the MISSING digit of
 *     the query path) whose output value is unpopulated.  STR keys are compared and ordered by dictionary id.  No key at all:
 *     one row, or none when nothing matches.
 *   aggregated columns: n_aggs (0..8) INT columns, each with a non-empty comma-separated subset of "n", "sum", "min", "max" in
 *     `ops`; anything else: SYBL_E_INVAL.  Every group keeps count (its matching rows) and, per aggregated column, n (the
 *     populated values), sum (the low 64 bits of the sum, as everywhere in the engine), min and max.  Unpopulated values
 *     contribute nothing.
 *   percentiles: `ops` also takes tokens p<k>, <k> a decimal integer 1..99 without a leading zero (so p0, p100, p05, p5.5 and p
 *     are refused, as are a token given twice and more than 8 percentile tokens on one column: SYBL_E_INVAL quoting the ops); a
 *     column may carry percentile tokens only ("p50").  With the group's n populated values of the column sorted ascending, p<k>
 *     is the element of 1-based rank ceil(k * n / 100), computed as (k * n + 99) / 100: nearest rank, no interpolation, exact at
 *     every int64 value.  n = 0: unpopulated, stored 0, exactly like _min / _max.  Filters, the time part, rows_no_time and the
 *     MISSING group behave as for the other aggregates.  The values are sorted on the GPU (one sort per column, shared by its
 *     percentiles; at most 2^31 - 1 values per column); sybl_table_rollup_pct_stats says how.
 *   output rows: one per distinct key among the kept rows, G of them, ascending lexicographically by (bucket, group 1, ..), an
 *     unpopulated value before every populated one.  The order does not depend on how workgroups were scheduled: two calls
 *     give identical tables.  Output block j = rows [j * block_rows, min(G, (j+1) * block_rows)); block_rows as for select.
 *   output columns, in this order: the time column, if bucketed (it keeps its name and holds bucket starts); the group columns
 *     by digest's rules (same name, type and IntInfo, dictionary id for id, the source's (width, base) -- every value is a
 *     source value --, a bitmap iff the MISSING group occurs); count_name (NULL / "" = "count"); per aggregated column, in the
 *     order named, those asked for of <col>_n, <col>_sum, <col>_min, <col>_max, then its <col>_p<k> in ascending k whatever
 *     their order in `ops`.  count and _n are always populated; _sum, _min, _max and _p<k> are unpopulated (stored 0) for a
 *     group with n = 0, and the column has a bitmap iff some group is so.  A name that collides: SYBL_E_INVAL naming it.
 *   storage of the new columns (time, count, aggregates): in compact mode by the storage rule over their exact output extrema
 *     (width 1, base 0 without a populated value), otherwise canonical.  Per-block statistics are exact for every column.
 *   limits: the mixed-radix composite key -- per key column the span of its tracked extrema (dictionary ids for STR, the
 *     quotients lo / B .. hi / B for the time part), plus one where the column has a bitmap, the time part most significant --
 *     must stay within 2^62: beyond, SYBL_E_INVAL saying so (a key column spanning the whole int64 range does that alone).  At
 *     most 2^27 cells or hash slots; a hash table that fills: SYBL_E_NOMEM.  N is unlimited.
 * The source is untouched and its version unmoved; the output owns everything and outlives it.  Rank-local, never collective
 * (across ranks: sybl_table_concat of the ranks' rollups, then a rollup of the sums -- percentiles do NOT merge that way: concat
 * the ranks' raw rows and roll those up); runs on the ctx stream, is complete on
 * return and thread-safe per ctx like select.  Any failure leaves *out NULL and sybl_last_error beginning
 * "sybl_table_rollup: "; when HBM runs out: SYBL_E_NOMEM, everything freed.
 * Out of scope: weights; histograms per group; interpolated or approximate percentiles, percentiles of STR or SET columns;
 * count distinct; SET keys; float averages (divide _sum by _n with
 * sybl_table_compute). */
typedef struct {
    const char *col;   /* an INT column */
    const char *ops;   /* e.g. "sum,max,p50,p99": a non-empty subset of n, sum, min, max and up to 8 of p1 .. p99 */
} sybl_rollup_agg;

typedef struct {
    int32_t n_filters;
    const sybl_filter *filters;
    int32_t n_groups;
    const char *const *groups;
    int32_t n_aggs;
    const sybl_rollup_agg *aggs;
    const char *time_col;     /* looked at when time_bucket > 0 */
    int64_t time_bucket;
    const char *count_name;
    int32_t block_rows;       /* 0 = 65536 */
} sybl_rollup_desc;

int sybl_table_rollup(sybl_table *t, const sybl_rollup_desc *d, sybl_table **out);

/* What the sybl_table_rollup that made this table did (zeros for any other table).  path: 1 = direct cells accumulated in
 * LDS, 2 = direct cells in HBM, 3 = hash; 0 = no kernel ran. */
typedef struct {
    int64_t rows_in;          /* N */
    int64_t rows_matched;     /* rows that passed the filters */
    int64_t rows_no_time;     /* ... of them dropped: time column unpopulated */
    int64_t groups;           /* G */
    int64_t blocks_out;
    int32_t path;
    int32_t fields;           /* int64 fields per cell: 1 + 4 per aggregated column */
    int64_t cells_or_slots;
    double filter_ms, accumulate_ms, order_ms, emit_ms;                  /* hipEvent time of the phases */
    int64_t filter_bytes, accumulate_bytes, order_bytes, emit_bytes;     /* computed from the shapes */
} sybl_rollup_stats;
int sybl_table_rollup_stats(const sybl_table *t, sybl_rollup_stats *out);

/* What the percentiles of the sybl_table_rollup that made this table cost (zeros for any table that no percentile rollup
 * made).  Per aggregated column with percentiles the populated values of the matching rows are sorted by cell << vbits |
 * (v - lo): as uint32 keys where the bits of the cells and of the value span fit 32 (variant32), as uint64 keys where they fit
 * 64 (variant64), otherwise by value and then stably by cell (variant_pairs).  A column none of whose values passed is not
 * sorted and counts in no variant. */
typedef struct {
    int32_t columns;          /* aggregated columns with at least one percentile */
    int32_t percentiles;      /* output columns made */
    int32_t variant32, variant64, variant_pairs;   /* columns sorted by each variant */
    int32_t key_bits_max;     /* the widest cell + value key */
    int64_t items;            /* values sorted, summed over the columns */
    double keys_ms, sort_ms, pick_ms;              /* hipEvent time, summed over the columns */
    int64_t keys_bytes, sort_bytes, pick_bytes;    /* computed from the shapes */
} sybl_rollup_pct_stats;
int sybl_table_rollup_pct_stats(const sybl_table *t, sybl_rollup_pct_stats *out);

/* Test hook (no GPU needed): the library's regular-expression engine for re / nre str filters -- Go regexp
 * (RE2) syntax, unanchored search like regexp.MatchString (filter.go:213-236).  1 = match, 0 = no match,
 * -1 = the pattern does not compile (sybl_last_error says why). */
int sybl_debug_regex_match(const char *pattern, const char *text, int64_t text_len);

/* Test hook (no GPU needed): regexp.ReplaceAllString(text, templ) of the same engine -- what -str-replace applies to
 * every dictionary string (column_store_io.go:517-530).  NULL = the pattern does not compile.  Library-owned buffer,
 * valid until the next call on the thread. */
const char *sybl_debug_regex_replace(const char *pattern, const char *text, const char *templ);

/* Test hooks (no GPU needed) for the count-distinct sketch: the host build of the very functions the kernel uses
 * (csrc/hll.h).  sybl_debug_hll_ints: rows of n_cols int64 values (row-major; populated: one byte per value, NULL = all
 * populated) pushed into `registers` (SYBL_HLL_REGISTERS bytes, updated in place) the way the int fast path does;
 * sybl_debug_hll_bytes: MetroHash64(seed 1337) of a byte string pushed the way the str path does, returns the hash;
 * sybl_debug_hll_cardinality: Cardinality() of a register array. */
int sybl_debug_hll_ints(const int64_t *values, const uint8_t *populated, int64_t n_rows, int32_t n_cols, uint8_t *registers);
uint64_t sybl_debug_hll_bytes(const uint8_t *bytes, int64_t len, uint8_t *registers);
int64_t sybl_debug_hll_cardinality(const uint8_t *registers);

/* Test/diagnostic hook: decodes one gob file (info.db, int_/str_/set_*.db, optionally .gz) to JSON
 * with the library's gob reader.  Library-owned buffer, valid until the next call on the thread. */
const char *sybl_debug_gob_to_json(const char *path);

/* Test/diagnostic hook: what the loader's worker half (no GPU involved) makes of ONE block directory -- the staging
 * slab it would send across PCIe -- as a text summary: the block's row count, per column its kind / element widths /
 * counts / extrema, and an FNV-1a digest of every region of the slab (bin values, bin offsets, record ids, values,
 * block-local ids, validity prefix) and of the block's string table.  types[i]: SYBL_INT_VAL / SYBL_STR_VAL /
 * SYBL_SET_VAL.  The CPU test suite holds the decode variants (AVX-512 windows / scalar loops, narrow / wide slices)
 * against each other with it.  NULL (and sybl_last_error) when the arguments are bad; an unreadable or broken block
 * is reported in the text.  Library-owned buffer, valid until the next call on the thread. */
const char *sybl_debug_block_layout(const char *block_dir, const char *const *columns, const int32_t *types, int32_t n_columns);

#ifdef __cplusplus
}
#endif
#endif /* SYBILGPU_H */
