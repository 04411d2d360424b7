/* hj3d.h — C ABI of the MI355X-native 3D hash-join engine (libhj3d.so).
 *
 * The reference (dflaxx/3d-hashjoin) has no FFI: its boundary is the compile-time
 * template surface of algebra.hh / ht_chaining.hh / ht_nested.hh. This ABI is what
 * that surface binds to. Each entry point replaces one reference interface:
 *
 *   hj3d_build  (HJ3D_CHAIN)   HtChaining1::insert            ht_chaining.hh:181-196
 *                              driven by AlgScan -> AlgHashJoinBuild::step  algebra.hh:259-269, 574-577
 *   hj3d_build  (HJ3D_NESTED)  HtNested1::insert              ht_nested.hh:287-311, 386-436
 *                              driven by AlgNestJoinBuild::step            algebra.hh:386-389
 *   hj3d_probe  (chain table)  AlgHashJoinProbe::step         algebra.hh:625-659
 *                              (+ HtChaining1::findDirEntryByOther ht_chaining.hh:236-248)
 *   hj3d_probe  (nested table) AlgNestJoinProbe::step         algebra.hh:435-459
 *                              (+ HtNested1::findMainNodeByOther ht_nested.hh:354-382)
 *                              and with HJ3D_PROBE_UNNEST also AlgUnnestHt::step  algebra.hh:510-541
 *   hj3d_probe2                the experiment-4 probe strand: two probes keyed on the same
 *                              probe attribute + deferred unnesting   main_experiment4.cc:831-1043
 *   hj3d_unnest                AlgUnnestHt::step as a separate operator over stored nested tuples
 *                              {a, main ref} (HJ3D_PROBE_MAINREF)     algebra.hh:490-541
 *   hj3d_unnest2               the two stacked unnests of experiment 4  main_experiment4.cc:435-466
 *   hj3d_probe_ref             AlgNestJoinProbe::step driven by another AlgNestJoinProbe: the probe
 *                              input is stored nested tuples           algebra.hh:435-459,
 *                                                                     main_experiment4.cc:847-850
 *   hj3d_probe_refn,           the two stacked to any depth up to HJ3D_NEST_MAX tables
 *   hj3d_unnestn                                                       algebra.hh:435-541
 *   hj3d_table_stats          HtChaining1/HtNested1::makeStatistics  ht_chaining.hh:260-292,
 *                                                                     ht_nested.hh:450-482
 *   hj3d_table_clear           HtChaining1/HtNested1::clear           ht_chaining.hh:250-258,
 *                                                                     ht_nested.hh:438-447
 *   hj3d_select                AlgSelection / AlgDynSelection::step   algebra.hh:278-358
 *   hj3d_probe_sel             AlgScan -> AlgSelection -> AlgHashJoinProbe / AlgNestJoinProbe
 *   hj3d_select_nested         AlgSelection / AlgDynSelection::step between AlgNestJoinProbe and
 *                              AlgUnnestHt, over stored nested tuples   algebra.hh:278-358 on 435-459,
 *                                                                     main_algebra_example.cc:226-234, 305-316
 *   hj3d_group_agg,            (no counterpart) aggregates over the rows stored nested tuples would unnest
 *   hj3d_agg_nested,           to, without running AlgUnnestHt::step   algebra.hh:490-541
 *   hj3d_agg_grouped           (per build group, per tuple or in total, per group of the join result)
 *
 * Semantics kept bit-exact with the reference: hash = murmur3 fmix32 (util/hasht.hh:52-61),
 * bucket = hash % num_buckets, and every counter the reference reports (match counts,
 * collision-chain comparisons c_htProbeCmp, unnest counts, HT statistics). The physical
 * layout is NOT the reference's pointer chains: tables are CSR-bucketized arrays, and the
 * reference's chain order (chaining: directory entry first, then newest-first; nested:
 * main nodes in first-occurrence order) is reproduced arithmetically from row ids.
 *
 * Join predicate: the engine joins on EQUALITY OF THE u32 JOIN ATTRIBUTE, tested as equality of
 * its fmix32 hash. fmix32 is a bijection on u32 (every step is invertible), so equal hashes are
 * equal keys and the reference's joinpred after the hash compare (algebra.hh:647-648) is implied
 * (SURVEY App. B item 7). A caller whose join predicate is anything else must not use this ABI;
 * the drop-in layer checks this on sample tuples (hj3d_host.hh check_joinpred) and refuses.
 *
 * Conventions: all relation/pair pointers are DEVICE pointers; every call is enqueued on the
 * context's stream (asynchronous) unless documented as synchronous. Calls return hj3d_status;
 * nothing throws. One host thread per context.
 */
#ifndef HJ3D_H
#define HJ3D_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  HJ3D_OK = 0,
  HJ3D_EINVAL = 1,       /* bad argument (null pointer, misaligned stride, ...)          */
  HJ3D_ENOMEM = 2,       /* device allocation failed                                      */
  HJ3D_EDEVICE = 3,      /* a HIP runtime call failed (see hj3d_last_error)               */
  HJ3D_EUNSUPPORTED = 4, /* a request outside what the engine implements                 */
  HJ3D_EOVERFLOW = 5     /* output buffer too small (counters are still complete)         */
} hj3d_status;

typedef struct hj3d_ctx hj3d_ctx;     /* device, stream, scratch arena, event timers        */
typedef struct hj3d_table hj3d_table; /* a device-resident hash table (chaining or nested)  */

#define HJ3D_ROW_IMPLICIT 0xFFFFFFFFu

/* A relation in device memory: array of structs. The join attribute is the u32 at
 * key_off of every tuple (main_experiment1.cc:86 tuple {k,a,b} -> stride 12, key_off 0 for
 * R.k, 4 for S.a). Row id of tuple i: row_base + i, or the u32 at row_off when
 * row_off != HJ3D_ROW_IMPLICIT (exchanged (key,row) pairs on multi-GPU). Row ids are the
 * identity of tuples: they are what the reference's tuple pointers become. The chain orders the
 * counters follow are derived from row order, so a build relation's explicit row ids must ascend in
 * its scan order (the reference's insertion order), as received pairs do: the exchange keeps each
 * source's pairs in row order and concatenates the sources in rank order. */
typedef struct {
  const void* base;
  uint64_t n;
  uint32_t stride;  /* bytes between consecutive tuples, multiple of 4, > 0 */
  uint32_t key_off; /* byte offset of the u32 join attribute, multiple of 4  */
  uint32_t row_off; /* byte offset of a u32 row id, or HJ3D_ROW_IMPLICIT     */
  uint32_t reserved;
  uint64_t row_base;
} hj3d_rel;

enum { HJ3D_CHAIN = 0, HJ3D_NESTED = 1 };

typedef struct {
  uint64_t num_buckets; /* global NB: bucket(key) = murmur32(key) % NB, 1 <= NB < 2^32     */
  uint64_t bucket_lo;   /* this table holds buckets [bucket_lo, bucket_hi) (a multi-GPU    */
  uint64_t bucket_hi;   /* shard); 0 / num_buckets on one GPU. Keys of other buckets are  */
                        /* ignored by build and never match in probe.                      */
  uint32_t kind;        /* HJ3D_CHAIN or HJ3D_NESTED                                        */
  uint32_t reserved;
} hj3d_table_desc;

/* probe flags */
#define HJ3D_PROBE_UNIQUE 0x1u /* IsBuildKeyUnique: stop at the first match (algebra.hh:653-655) */
#define HJ3D_PROBE_UNNEST 0x2u /* nested table: expand main + sub-chain (AlgUnnestHt)           */
#define HJ3D_PROBE_EMIT   0x4u /* write output tuples to out_dev (else aggregate only)          */
#define HJ3D_PROBE_ACCUMULATE 0x10u /* add to the result slot of the previous probe instead of
                                       restarting it (one probe strand issued in chunks) */
#define HJ3D_PROBE_CHECKSUM 0x8u /* fold sum_a/sum_b/sum_h/xor_h over the output (verification;
                                    the reference itself only counts); counts are always exact */
/* HJ3D_PROBE_MAINREF: the nested result tuple carries its group, as AlgNestJoinProbe's output
 * {probe tuple, MainNode*} does (algebra.hh:435-459). Nested table only, with HJ3D_PROBE_EMIT and
 * without HJ3D_PROBE_UNNEST (anything else: HJ3D_EINVAL). The dense output slot of a probe tuple is
 * then {u32 probe row, u32 main_ref}: main_ref = the index of the matched main record in the table's
 * main-record array (the index into hj3d_table_export's `payload`), 0xFFFFFFFF without a match.
 * Counters and checksums are those of the probe without the flag (sum_b / sum_h / xor_h fold the first
 * build row). hj3d_unnest / hj3d_unnest2 expand such refs later. A ref is valid until the table's next
 * hj3d_build, hj3d_build_many or hj3d_table_clear. */
#define HJ3D_PROBE_MAINREF 0x20u

/* Result of one probe strand. Orientation follows the reference's concat functors:
 * a = probe-side row, b = build-side row (for a nested probe without unnest, b = the row of
 * the matched key's first build tuple, i.e. MainNode::data()). */
typedef struct {
  uint64_t n_probe;   /* probe tuples scanned                    (c_scanProbe)             */
  uint64_t n_matched; /* probe tuples with >= 1 match            (nested c_htProbe)         */
  uint64_t n_out;     /* output tuples: chaining c_htProbe, nested c_unnest / c_top         */
  uint64_t n_cmps;    /* collision-chain comparisons             (c_htProbeCmp, bit-exact)  */
  uint64_t sum_a, sum_b, sum_c; /* sum of row ids over output tuples (c only for triples)   */
  uint64_t sum_h, xor_h;        /* sum / xor of HJ3D pair (triple) hashes over output tuples */
} hj3d_probe_res;

/* Result of the experiment-4 probe strand (main_experiment4.cc:831-1043 counter columns).
 * Output triples (r, s, t) rows; a = r, b = s, c = t in the checksums. */
typedef struct {
  uint64_t c_probe_rs, c_probe_rs_cmp, c_probe_rt, c_probe_rt_cmp;
  uint64_t c_unnest_1, c_unnest_2, c_top;
  uint64_t sum_a, sum_b, sum_c, sum_h, xor_h;
} hj3d_probe2_res;

/* HtStatistics (ht_statistics.hh:18-54): cc0 over all buckets, cc1 over non-empty ones.
 * Chain length = #entries (chaining) or #main nodes = distinct keys (nested) per bucket. */
typedef struct {
  uint64_t nb, empty, entries, distinct;
  uint64_t cc0_min, cc0_max, cc0_sum, cc0_cnt;
  uint64_t cc1_min, cc1_max, cc1_sum, cc1_cnt;
} hj3d_stats;

/* ---- checksums (definitions shared with oracle/ and tests) ----
 * mix64 = splitmix64 finalizer; pair(a,b) = mix64(a<<32 | b); triple(a,b,c) = mix64(pair(a,b) ^ c) */
uint64_t hj3d_mix64(uint64_t z);

/* ---- context ---- */
/* hip_stream: the stream every call of this context is enqueued on; NULL = the device's null
 * (default) stream, i.e. the stream torch uses unless told otherwise. */
hj3d_status hj3d_ctx_create(int device, void* hip_stream, hj3d_ctx** out);
void        hj3d_ctx_destroy(hj3d_ctx* ctx);
/* Later calls are enqueued on hip_stream (NULL: the null stream). The call inserts NO ordering between
 * the old and the new stream: work enqueued before it stays on the old stream, and nothing on the new
 * stream waits for it. Before a call on the new stream uses what calls on the old one produced (a built
 * table, the result slot, the context's scratch), the caller orders the new stream after the old one
 * (an event recorded on the old and waited for on the new stream, or hj3d_ctx_sync before the switch).
 * A nested build still pending is finished by a host wait on the build's own event, so its counts are
 * safe; the table's device arrays are not. hj3d_ctx_stream returns the current handle. */
hj3d_status hj3d_ctx_set_stream(hj3d_ctx* ctx, void* hip_stream);
void*       hj3d_ctx_stream(const hj3d_ctx* ctx);
hj3d_status hj3d_ctx_sync(hj3d_ctx* ctx); /* synchronous: waits for the stream */
const char* hj3d_last_error(const hj3d_ctx* ctx);
/* Engine options. HJ3D_OPT_FORCE_DIRECT (0/1): probe / build the chaining table without the
 * radix-partitioned (LDS-slice) kernels, i.e. with one random table access chain per tuple
 * (kept for small inputs and for A/B measurements). */
enum {
  HJ3D_OPT_FORCE_DIRECT = 1,
  /* HJ3D_OPT_RADIX_MIN (tuples): probes of at least this many tuples (builds of at least 1/16 of
   * it) use the radix-partitioned kernels; default 2^20. */
  HJ3D_OPT_RADIX_MIN = 2,
  /* 3: reserved (a nested build from the radix bucket CSR with per-bucket key grouping: faster at low
   * bucket fill, slower under Zipf skew than the aggregation build; removed in round 6) */
  /* HJ3D_OPT_NESTED_SORT (0/1, default 0): build nested tables by the LSD key sort (nested.hip)
   * instead of the bucket-range partition + per-partition LDS aggregation (nested_agg.hip, the
   * default for large inputs). */
  HJ3D_OPT_NESTED_SORT = 4,
  /* HJ3D_OPT_SEL_UNFUSED (0/1, default 0): hj3d_probe_sel always selects first (hj3d_select) and
   * probes the passing pairs, instead of fusing the selection into the probe partitioner. */
  HJ3D_OPT_SEL_UNFUSED = 5,
  /* HJ3D_OPT_PACKED_PROBE (0/1, default 1): the unique chaining probe partitions the probe side into
   * packed {bucket-in-slice | hash / NB, row} pairs and finishes in two launches; 0 keeps the
   * {hash, row} partitioned probe (A/B measurements). */
  HJ3D_OPT_PACKED_PROBE = 6,
  /* HJ3D_OPT_PROBE_ITEMS (0 or 5..8, default 0): pairs per lane and chunk in the packed probe's
   * region walk; 0 picks it from the expected region length (tests and A/B measurements). */
  HJ3D_OPT_PROBE_ITEMS = 7,
  /* HJ3D_OPT_PK_SLICE (buckets, 0 or >= 2; default 0): upper bound on the packed probe's slice
   * width (normally the largest that fits one workgroup's LDS). Tables of more than 1024 slices
   * take the two-level partition (k_pk_part into coarse ranges, k_pk_split by slice), so a small
   * bound puts small tables on that path (tests). It bounds the partitioned nested probe's slice
   * width too: beyond 2048 slices that probe takes the same two-level partition. */
  HJ3D_OPT_PK_SLICE = 8,
  /* HJ3D_OPT_PK_STAGE (pairs, default 0 = the whole LDS stage): the packed partitioner's stage form
   * (two slices per thread: more than 1024 slices in one partition level) writes its carried partial
   * segments out early once the carries plus a tile exceed this many pairs (tests: 1 flushes after
   * every tile). The window form (up to 1024 slices) carries nothing and ignores it. */
  HJ3D_OPT_PK_STAGE = 9,
  /* HJ3D_OPT_PK_BUILD (0/1, default 0): chaining builds take the slice build of tables beyond the
   * radix build's range (R through the packed partitioner's two levels into 8192-bucket slices,
   * each built in LDS; synchronous, region overflow falls back to the direct build) whenever it
   * applies, not only above 2048 x 16384 buckets (tests). */
  HJ3D_OPT_PK_BUILD = 10,
  /* HJ3D_OPT_NESTED_PK (0/1, default 0): the nested aggregation build partitions by the packed
   * partitioner's slices (k_pk_part + k_pk_split, the form tables of more than 2048 partitions take,
   * e.g. config D's 1e8-bucket Nrs table) whenever it applies, not only above 2048 partitions
   * (tests). Region overflow (skewed keys) falls back to the sort build. */
  HJ3D_OPT_NESTED_PK = 11,
  /* 12: reserved (a compact slice image for the packed probe, measured slower: 0.61 against 0.49 ms
   * at config B; removed in round 6) */
  /* HJ3D_OPT_SYNC_BUILD (0/1, default 0): hj3d_build / hj3d_build_many finish a nested table before
   * they return (they wait for its counts and run the sort build there if the LDS aggregation build
   * gave up), so the build relation's device memory may be released as soon as the call returns.
   * Default: the table finishes at its next use (see hj3d_build). */
  HJ3D_OPT_SYNC_BUILD = 13,
  /* 14: retired (the two-level nested partition, measured slower than the one-level one) */
  /* HJ3D_OPT_RP_UNFUSED (0/1, default 0): small implicit-row partitions of chaining builds run as
   * two launches (histogram, then scatter) instead of the fused one-launch partition with its grid
   * barrier (A/B measurements and the parity test of both forms). Nested builds always take the two
   * launches: the barrier's timeout flag lives in a word of the table that a nested table uses for
   * its own build. The fused form runs only when the
   * occupancy API confirms all its workgroups are resident (another stream holding CUs can still
   * delay some); should a barrier not complete within 0.2 s, its workgroups go on with partial
   * partition sizes and the table is invalid: hj3d_table_stats / _size / _export / _finish of that
   * table and the next hj3d_probe_result / hj3d_probe2_result return HJ3D_EDEVICE. A rebuild of the
   * table replaces it. */
  HJ3D_OPT_RP_UNFUSED = 15,
  /* HJ3D_OPT_DIAG_GBAR (ticks of the 100 MHz clock, default 0 = off): diagnostic for the failure path
   * above. The fused partition's barrier then times out after this many ticks, and its workgroup 0
   * never arrives, so every barrier of such a build times out (tests). Chaining builds only: no
   * nested build takes the fused partition. */
  HJ3D_OPT_DIAG_GBAR = 16,
  /* HJ3D_OPT_DIAG_LOOKBACK (ticks of the 100 MHz clock, default 0 = off): diagnostic of the nested
   * build on the packed slices (the aggregation form that finishes by decoupled look-back: each
   * partition's main-record base waits on its predecessors' published counts, at most 0.2 s, after
   * which the build gives up and the sort build replaces the table). Partition 0 then never
   * publishes and the wait limit is this many ticks, so every such build gives up (tests). */
  HJ3D_OPT_DIAG_LOOKBACK = 17,
  /* HJ3D_OPT_GBY_FORM (0..3, default 0): which kernel form hj3d_agg_grouped takes. 0 = chosen per call;
   * 1 = direct (one global atomic per live tuple and spec); 2 = the whole column kept in LDS by every
   * workgroup (when it does not fit: form 1); 3 = a direct-mapped LDS cache of groups in front of the
   * global atomics. Every form gives the same column (tests and A/B). */
  HJ3D_OPT_GBY_FORM = 18
};
hj3d_status hj3d_ctx_set_option(hj3d_ctx* ctx, int option, int64_t value);
/* Timing events for a host's own phase timers (the bench's build / probe boundaries): HIP events
 * created without the system-scope fence (hipEventDisableSystemFence), recorded on the context
 * stream. A default event writes the L2 back when it is recorded, which leaves the GPU idle
 * ~10 us between the kernels around it. hj3d_tevent_elapsed waits for b, then gives b - a in ms. */
hj3d_status hj3d_tevent_create(hj3d_ctx* ctx, void** ev);
hj3d_status hj3d_tevent_record(hj3d_ctx* ctx, void* ev);
hj3d_status hj3d_tevent_elapsed(void* a, void* b, float* ms);
void hj3d_tevent_destroy(void* ev);
/* Kernel-phase timers: HIP events recorded on the context stream around every phase
 * (phase ids below). hj3d_ctx_timer reads (synchronously) the summed milliseconds and the
 * number of recorded intervals since the last reset. hj3d_ctx_timing(ctx, mode): 0 off; 1 every
 * timer (whole-call phases are marker events between the kernels on the stream); 2 only the timers
 * whose events travel with a kernel's dispatch (the packed probe's k_pk_part / k_pk_split /
 * k_pk_probe), so timing puts no packet between the kernels. */
enum {
  HJ3D_T_BUILD = 0,         /* hj3d_build, whole call */
  HJ3D_T_PROBE = 1,         /* hj3d_probe / hj3d_probe2, whole call */
  HJ3D_T_PROBE_KERNEL = 2,  /* the join-probe kernel launches only (radix path: k_rp_probe) */
  HJ3D_T_PARTITION = 3,     /* hj3d_partition (multi-GPU exchange partitioner) */
  HJ3D_T_SCATTER = 4,       /* radix probe path: probe-side partition scatter kernel */
  HJ3D_T_HIST = 5,          /* radix probe path: probe-side partition histogram kernel; packed probe
                             * of more than 1024 slices: its second partition level (k_pk_split) */
  HJ3D_T_NTIMERS = 6
};
/* Kernel launches issued by this library so far, all contexts of the process (diagnostic: the bench
 * reports launches per step). */
uint64_t hj3d_launch_count(void);
/* Diagnostic: per-partition phase clocks of the last k_nagg launch (library built with
 * -DHJ3D_NAGG_CLK=1; otherwise HJ3D_EUNSUPPORTED). 8 u64 words per partition: 0 entry, 1 table
 * cleared, 2 pass A done, 3 main records written, 4 pass B done, 5 exit (100 MHz wall clock), 7 the
 * workgroup's dispatch index. parts <= 16384. */
hj3d_status hj3d_diag_nagg_clk(uint64_t* host, uint32_t parts);
hj3d_status hj3d_ctx_timing(hj3d_ctx* ctx, int mode);
hj3d_status hj3d_ctx_timer(hj3d_ctx* ctx, int phase, double* ms_total, uint64_t* count);
hj3d_status hj3d_ctx_timer_reset(hj3d_ctx* ctx);

/* ---- device memory for hosts that link only this ABI (the C++ drop-in layer) ---- */
hj3d_status hj3d_dev_alloc(hj3d_ctx* ctx, uint64_t bytes, void** dev);
hj3d_status hj3d_dev_free(hj3d_ctx* ctx, void* dev);
/* synchronous copies (host <-> device) on the context stream */
hj3d_status hj3d_upload(hj3d_ctx* ctx, void* dev, const void* host, uint64_t bytes);
hj3d_status hj3d_download(hj3d_ctx* ctx, void* host, const void* dev, uint64_t bytes);

/* ---- tables ---- */
hj3d_status hj3d_table_create(hj3d_ctx* ctx, const hj3d_table_desc* desc, hj3d_table** out);
void        hj3d_table_destroy(hj3d_table* t);
/* Pre-size device storage for builds of up to max_build tuples (allocation outside timed loops). */
hj3d_status hj3d_table_reserve(hj3d_ctx* ctx, hj3d_table* t, uint64_t max_build);
/* Empties the table (asynchronous); its device storage is kept. Afterwards the table is in the state
 * of one never built: hj3d_table_build_path is "none", every getter succeeds (hj3d_table_export gives
 * n_payload = n_sub = 0 and all-zero offsets, the statistics are those of an empty table), and probes
 * are valid and match nothing (n_probe = the probe tuples, every other counter 0; a dense EMIT output
 * carries 0xFFFFFFFF in every slot). A build in flight for the old content is dropped. */
hj3d_status hj3d_table_clear(hj3d_ctx* ctx, hj3d_table* t);
/* Build: replaces the table content with the tuples of `build` (asynchronous). A nested table's
 * build finishes at the table's next use (probe, statistics, export): its counts are read then, and
 * when the LDS aggregation build gave up on a key range too dense for it, the sort build runs then,
 * from `build` again -- so the build relation's device memory must stay valid until that use (or set
 * HJ3D_OPT_SYNC_BUILD). That fallback build is timed as HJ3D_T_BUILD, not as part of the probe. */
hj3d_status hj3d_build(hj3d_ctx* ctx, hj3d_table* t, const hj3d_rel* build);
/* Builds several tables, tables[k] from builds[k] (asynchronous; as hj3d_build for each). Two nested
 * tables of one geometry (equal num_buckets and bucket range: experiment 4's S and T tables,
 * main_experiment4.cc:832-859) take ONE launch sequence: both relations partitioned, one
 * aggregation grid over both tables' partitions, one scan, one compaction. Otherwise the tables
 * are built one after another. Replaces the reference's consecutive AlgScan -> AlgNestJoinBuild
 * runs (main_experiment4.cc:856-859, 879-881). */
hj3d_status hj3d_build_many(hj3d_ctx* ctx, hj3d_table* const* tables, const hj3d_rel* builds, uint32_t count);
/* Host copy of a table's device arrays (synchronous): what the drop-in layer's per-tuple probes
 * walk (HtChaining1::findDirEntryByOther ht_chaining.hh:236-248, HtNested1::findMainNodeByOther
 * ht_nested.hh:354-382). Call with NULL arrays first to get the sizes: *n_payload = entries
 * (chaining) or main records (nested), *n_sub = the extent of a nested table's row array `sub` (0
 * for chaining): the tuple count of the build relation, so at least the stored rows.
 * Then off[nb_local + 1] receives the CSR offsets of the local buckets into the payload, payload
 * the chaining entries {u32 hash, u32 row} or the nested main records {u32 hash, first_row,
 * sub_off, sub_len}, and sub (nested) the build rows grouped per key, sub[sub_off .. + sub_len).
 * The main records' ranges are pairwise disjoint and lie inside [0, n_sub); their lengths add up to
 * the stored rows (hj3d_stats.entries). For a table that stores every build tuple they tile
 * [0, n_sub) exactly. A bucket-range shard fed tuples of other buckets leaves n_sub - entries
 * positions outside every range: the sort build keeps the unowned tuples' rows there, the aggregation
 * builds pack the stored rows at the front and leave the tail unwritten. No main record refers to
 * them; a consumer reads sub only through the ranges.
 * Entry order: chaining buckets of <= 32 entries come sorted by row (the reference's chain order is
 * then [first, newest, ..., second], arithmetic in that order); longer buckets are in no defined
 * order (the builds claim their runs with atomics) -- a consumer that needs the reference's chain
 * order there sorts by row, as the drop-in host view does. Nested: mains and sub rows in no defined
 * order (the reference's order follows from first_row and the rows). */
hj3d_status hj3d_table_export(hj3d_ctx* ctx, const hj3d_table* t, uint32_t* off, void* payload, uint32_t* sub,
                              uint64_t* n_payload, uint64_t* n_sub);
/* Which build made the table's current content (diagnostic, static string): chaining "radix",
 * "slices" (pk_slices, tables beyond the radix build's range) or "direct"; nested "nested_agg",
 * "nested_agg_slices" (more than 2048 partitions), each with "_reg" appended when the register form
 * aggregated them, or "nested_sort"; "none" before a
 * build and after hj3d_table_clear. A nested table whose build has not been resolved yet (no use since hj3d_build) reports the
 * path that was started, with "?" appended ("nested_agg?"): the getter never waits or builds. Replaces
 * nothing of the reference (which has one insert path). */
const char* hj3d_table_build_path(const hj3d_table* t);
/* Finishes a nested table's build now (waits for its counts; runs the sort build from the build
 * relation if the LDS aggregation build gave up), as its next use would. No-op for a finished table.
 * Replaces nothing of the reference (whose insert is synchronous). */
hj3d_status hj3d_table_finish(hj3d_ctx* ctx, hj3d_table* t);
/* Synchronous statistics (makeStatistics). */
hj3d_status hj3d_table_stats(hj3d_ctx* ctx, const hj3d_table* t, hj3d_stats* out);
/* Number of tuples / distinct keys currently stored (synchronous). */
hj3d_status hj3d_table_size(hj3d_ctx* ctx, const hj3d_table* t, uint64_t* n_entries, uint64_t* n_distinct);

/* ---- probe ----
 * Asynchronous: counters accumulate in a device-side result slot; hj3d_probe_result reads it
 * (synchronous). With HJ3D_PROBE_EMIT, output pairs {u32 a, u32 b} are written to out_dev
 * (at most out_cap pairs; n_out still counts all and HJ3D_EOVERFLOW is reported by
 * hj3d_probe_result if n_out > out_cap). Pair order in out_dev is unspecified. */
hj3d_status hj3d_probe(hj3d_ctx* ctx, const hj3d_table* t, const hj3d_rel* probe, uint32_t flags,
                       void* out_dev, uint64_t out_cap);
hj3d_status hj3d_probe_result(hj3d_ctx* ctx, hj3d_probe_res* out);

/* Experiment-4 probe strand over two tables built on S and T (both HJ3D_NESTED: Ndu with deferred
 * unnesting; both HJ3D_CHAIN: Chj). With HJ3D_PROBE_EMIT, the output triples go to out_dev as an array
 * of {u32 r_row, u32 s_row, u32 t_row} (12 bytes each, out_dev 4-byte aligned), at most out_cap of
 * them, in no specified order (it differs from run to run); nothing is written at or beyond
 * out_dev + 12 * out_cap. c_top and every other counter and checksum still count all triples, and
 * hj3d_probe2_result returns HJ3D_EOVERFLOW (with the complete counters) if c_top > out_cap; the
 * out_cap triples written are then some out_cap of the result. EMIT with out_dev == NULL and
 * out_cap > 0, and EMIT with HJ3D_PROBE_ACCUMULATE (the strand has no accumulate form; without EMIT
 * that flag is ignored), are HJ3D_EINVAL. Replaces the two unnest functors of
 * main_experiment4.cc:435-466 filling result_tuple_t.
 * The row sums sum_a / sum_b / sum_c are always folded (the unnest reads every output triple's
 * rows); the triple hashes sum_h / xor_h only with HJ3D_PROBE_CHECKSUM (else 0), with or without EMIT. */
hj3d_status hj3d_probe2(hj3d_ctx* ctx, const hj3d_table* ts, const hj3d_table* tt, const hj3d_rel* probe,
                        uint32_t flags, void* out_dev, uint64_t out_cap);
hj3d_status hj3d_probe2_result(hj3d_ctx* ctx, hj3d_probe2_res* out);

/* ---- deferred unnesting as operators of their own ----
 * hj3d_unnest replaces AlgUnnestHt::step (algebra.hh:490-541) stacked anywhere downstream of a nested
 * probe (main_algebra_example.cc:305-316). nested_dev: n stored nested tuples {u32 a, u32 main_ref}
 * (8 bytes each) in device memory: what a HJ3D_PROBE_MAINREF probe of `t` wrote, possibly filtered,
 * reordered or concatenated since. A tuple whose ref is 0xFFFFFFFF (no match), or not below the
 * table's current main-record count (the table was cleared or rebuilt smaller since the probe), is
 * skipped; no memory is read through such a ref. Every other tuple yields {a, row} for each build row
 * of main record main_ref (sub[sub_off .. sub_off + sub_len)): with HJ3D_PROBE_EMIT, pairs
 * {u32 a, u32 build row} to out_dev, at most out_cap of them, in no specified order; nothing is
 * written at or beyond out_dev + 8 * out_cap. Without EMIT only the counters and sums are computed.
 * flags: HJ3D_PROBE_EMIT and HJ3D_PROBE_CHECKSUM only. HJ3D_EINVAL: any other flag, a chaining
 * table, EMIT with out_dev == NULL and out_cap > 0, n >= 2^32. Asynchronous; a nested build still
 * pending is finished first, as by a probe. The result goes to the probe result slot
 * (hj3d_probe_result): n_probe = n, n_matched = tuples with a valid ref, n_out = output pairs
 * (c_unnest), n_cmps = 0, sum_a / sum_b always, sum_h / xor_h only with HJ3D_PROBE_CHECKSUM (else 0);
 * HJ3D_EOVERFLOW (with the complete counters) if n_out > out_cap. */
hj3d_status hj3d_unnest(hj3d_ctx* ctx, const hj3d_table* t, const void* nested_dev, uint64_t n, uint32_t flags,
                        void* out_dev, uint64_t out_cap);
/* hj3d_unnest2 replaces the two stacked unnest functors of experiment 4 (main_experiment4.cc:435-466)
 * without hj3d_probe2's restriction to one probe attribute: nested_dev holds n triples
 * {u32 a, u32 ref_s, u32 ref_t} (12 bytes each, 4-byte aligned), ref_s a main ref of ts and ref_t one
 * of tt (both HJ3D_NESTED; their geometries may differ). A triple with an invalid ref (the rule of
 * hj3d_unnest, per table) is skipped; every other yields {a, s_row, t_row} for each combination of the
 * two groups' rows. Output layout, capacity rule and order as hj3d_probe2 with HJ3D_PROBE_EMIT.
 * flags: HJ3D_PROBE_EMIT and HJ3D_PROBE_CHECKSUM only; HJ3D_EINVAL as for hj3d_unnest. The result
 * goes to the hj3d_probe2 result slot (hj3d_probe2_result): c_unnest_1 = sum of |T group| (the
 * reference unnests T first), c_unnest_2 = c_top = sum of |S group| * |T group|, c_probe_* = 0,
 * sum_a / sum_b / sum_c always, sum_h / xor_h only with HJ3D_PROBE_CHECKSUM; HJ3D_EOVERFLOW (complete
 * counters) if c_top > out_cap. */
hj3d_status hj3d_unnest2(hj3d_ctx* ctx, const hj3d_table* ts, const hj3d_table* tt, const void* nested_dev,
                         uint64_t n, uint32_t flags, void* out_dev, uint64_t out_cap);
/* hj3d_probe_ref: the chained nested probe. Replaces AlgNestJoinProbe::step (algebra.hh:435-459) driven
 * by another AlgNestJoinProbe, i.e. the second probe of experiment 4's strand, whose input is the first
 * probe's nested output (probe_RS_t over probe_RT_t, main_experiment4.cc:847-850), without
 * hj3d_probe2's restriction to one probe attribute: probe -> probe_ref -> ... -> unnest runs an n-way
 * nested join on different attributes on the device.
 * nested_dev: n stored nested tuples of in_words u32 words each (4-byte aligned): {a} (in_words 1) or
 * {a, ref} (in_words 2: what a HJ3D_PROBE_MAINREF probe wrote, its dense output as it stands,
 * 0xFFFFFFFF refs included, or filtered, reordered or concatenated since). a is a row id of `base`, the
 * probe-side relation (implicit rows: tuple index a - base->row_base); the join key is the u32 at
 * base->key_off of that tuple. A tuple is live iff a is a row of base and (in_words 2) its ref is not
 * 0xFFFFFFFF. A dead tuple is skipped, as AlgNestJoinProbe passes nothing downstream without a match:
 * not probed, not counted, and no memory is read through it. Carried refs are opaque: copied, never
 * dereferenced. Every live tuple probes `t` (HJ3D_NESTED) with its key, each occurrence of a row on
 * its own (a tuple is identified by its position in the input, not by a).
 * With HJ3D_PROBE_EMIT every live tuple that finds its key yields one tuple of in_words + 1 words, the
 * input tuple followed by the main_ref of t (as HJ3D_PROBE_MAINREF): compact, in no specified order,
 * at most out_cap of them; nothing is written at or beyond out_dev + 4 * (in_words + 1) * out_cap. The
 * output feeds hj3d_unnest (in_words 1), hj3d_unnest2 (in_words 2) or another hj3d_probe_ref.
 * Result (hj3d_probe_result): n_probe = live tuples, n_matched = n_out = live tuples with a match,
 * n_cmps = the collision-chain comparisons of exactly those probes (bit-exact: what hj3d_probe reports
 * for a relation of the live tuples' keys), sum_a = the sum of a over the output tuples (always); with
 * HJ3D_PROBE_CHECKSUM sum_b = the sum of the matched main records' first build rows and sum_h / xor_h
 * fold pair(a, first build row) (else 0); sum_c = 0. HJ3D_EOVERFLOW (complete counters) if
 * n_out > out_cap. A cleared table gives n_probe = live tuples and every other counter 0.
 * flags: HJ3D_PROBE_EMIT and HJ3D_PROBE_CHECKSUM only. HJ3D_EINVAL: any other flag, a null ctx / t /
 * base, a chaining table, in_words not 1 or 2, EMIT with out_dev == NULL and out_cap > 0, nested_dev or
 * out_dev not 4-byte aligned, n && !nested_dev, n >= 2^32, an invalid base or one with explicit rows.
 * nested_dev and out_dev must not overlap. A nested build still pending is finished first, as by a
 * probe. Runs as hj3d_probe_sel over a staged relation of the tuples' keys (all probe paths apply):
 * asynchronous on the partitioned probe path, where the liveness test is fused into the probe
 * partitioner; otherwise the call waits for the stream once (the live count is read). */
hj3d_status hj3d_probe_ref(hj3d_ctx* ctx, const hj3d_table* t, const hj3d_rel* base, const void* nested_dev,
                           uint64_t n, uint32_t in_words, uint32_t flags, void* out_dev, uint64_t out_cap);

/* ---- wide nested tuples: the chain probe -> probe_refn -> .. -> unnestn over up to HJ3D_NEST_MAX tables ----
 * AlgNestJoinProbe / AlgUnnestHt stack to any depth (algebra.hh:435-541); experiment 4 is the depth-2
 * instance (main_experiment4.cc:435-466, 847-850). A stored nested tuple {a, ref_1 .. ref_k} carries at
 * most HJ3D_NEST_MAX main refs. */
#define HJ3D_NEST_MAX 6 /* main refs a stored nested tuple may carry */

/* hj3d_probe_refn: hj3d_probe_ref for tuples of 1..HJ3D_NEST_MAX words {a, ref_1 .. ref_{in_words-1}}, so
 * that its output (in_words + 1 <= 7 words) feeds it again. The contract is hj3d_probe_ref's, except:
 * in_words ranges over 1 .. HJ3D_NEST_MAX (anything else: HJ3D_EINVAL); a tuple is live iff a is a row of
 * base and none of its carried refs is 0xFFFFFFFF; every carried ref is opaque (copied, never
 * dereferenced). Counters, checksums, overflow rule, asynchrony and result slot (hj3d_probe_result) are
 * hj3d_probe_ref's; n_cmps is bit-exact. The output feeds hj3d_unnestn (k = in_words) or another
 * hj3d_probe_refn. hj3d_probe_ref itself keeps refusing in_words > 2. */
hj3d_status hj3d_probe_refn(hj3d_ctx* ctx, const hj3d_table* t, const hj3d_rel* base, const void* nested_dev,
                            uint64_t n, uint32_t in_words, uint32_t flags, void* out_dev, uint64_t out_cap);

/* Result of hj3d_unnestn over k tables; the counters follow the reference's order, in which the last
 * table probed is unnested first (main_experiment4.cc:435-466). With |G_i| the group of a tuple's ref_i:
 * c_unnest[j] (j < k) = the outputs of the (j + 1)-th unnest executed = sum over the live tuples of
 * |G_k| * .. * |G_{k-j}|; entries j >= k are 0; c_top = c_unnest[k - 1]. For k = 2 these are
 * hj3d_unnest2's c_unnest_1 / c_unnest_2. sum_row[i - 1] = the sum of row_i over the output rows. */
typedef struct {
  uint64_t n_in, n_live;            /* tuples given / tuples with every ref valid */
  uint64_t c_unnest[HJ3D_NEST_MAX];
  uint64_t c_top;
  uint64_t sum_a, sum_row[HJ3D_NEST_MAX], sum_h, xor_h;
} hj3d_unnestn_res;

/* hj3d_unnestn: k stacked unnests (AlgUnnestHt::step, algebra.hh:490-541) as one operator, the k-table
 * form of hj3d_unnest (k = 1) and hj3d_unnest2 (k = 2). nested_dev holds n tuples {u32 a, u32 ref_1 ..
 * ref_k} of k + 1 words (4-byte aligned), ref_i a main ref of tables[i - 1]. Every table is HJ3D_NESTED;
 * their geometries are free and a table may appear more than once (self joins). A tuple with any ref not
 * below its table's current main-record count is skipped and no memory is read through it (the rule of
 * hj3d_unnest, per table). Every other tuple yields {a, row_1 .. row_k} for each combination of the k
 * groups' rows: with HJ3D_PROBE_EMIT as rows of 4 (k + 1) bytes to out_dev, at most out_cap of them, in
 * no specified order; nothing is written at or beyond out_dev + 4 (k + 1) out_cap.
 * The result goes to a slot of its own (hj3d_unnestn_result; the probe result slots are not touched):
 * sum_a and sum_row always; with HJ3D_PROBE_CHECKSUM sum_h / xor_h fold h = pair(a, row_1), then
 * h = mix64(h ^ row_i) for i = 2..k (the pair hash for k = 1, the triple hash for k = 2), else 0.
 * hj3d_unnestn_result returns HJ3D_EOVERFLOW (with the complete counters) if c_top > out_cap under EMIT.
 * Counts are exact while every tuple's product |G_1| * .. * |G_k| and c_top stay below 2^63; otherwise
 * hj3d_unnestn_result returns HJ3D_EUNSUPPORTED (only n_in and n_live are set) and no output row was written.
 * flags: HJ3D_PROBE_EMIT and HJ3D_PROBE_CHECKSUM only. HJ3D_EINVAL: any other flag, a null ctx / tables /
 * entry of tables, a chaining table, k outside 1 .. HJ3D_NEST_MAX, n && !nested_dev, nested_dev or out_dev
 * not 4-byte aligned, EMIT with out_dev == NULL and out_cap > 0, n >= 2^32; hj3d_unnestn_result before any
 * hj3d_unnestn. Asynchronous; nested builds still pending are finished first, as by a probe. */
hj3d_status hj3d_unnestn(hj3d_ctx* ctx, const hj3d_table* const* tables, uint32_t k, const void* nested_dev,
                         uint64_t n, uint32_t flags, void* out_dev, uint64_t out_cap);
hj3d_status hj3d_unnestn_result(hj3d_ctx* ctx, hj3d_unnestn_res* out);

/* ---- multi-GPU exchange helpers (bucket-range radix partition) ----
 * Destination of a tuple: owner(bucket) = bucket * nparts / num_buckets. Writes (key,row)
 * pairs grouped by destination into out_pairs_dev (capacity rel->n pairs) and the per
 * destination counts into counts_dev[nparts] (device u64). Order within a destination
 * follows input order (stable). */
hj3d_status hj3d_partition(hj3d_ctx* ctx, const hj3d_rel* rel, uint64_t num_buckets, uint32_t nparts,
                           void* out_pairs_dev, void* counts_dev);
/* The same with a selection below the exchange (AlgSelection, algebra.hh:278-358): only the tuples
 * passing the predicate conjunction (hj3d_sel_pred, below) are partitioned and shipped; row ids
 * stay those of `rel`, so the probe downstream reports the reference's rows. */
typedef struct hj3d_sel_pred hj3d_sel_pred;
hj3d_status hj3d_partition_sel(hj3d_ctx* ctx, const hj3d_rel* rel, const hj3d_sel_pred* preds, uint32_t npred,
                               uint64_t num_buckets, uint32_t nparts, void* out_pairs_dev, void* counts_dev);
/* Single-pass form for the probe side of the exchange (no order kept inside a destination: the
 * probe's counters are per tuple; the build side keeps hj3d_partition's stable order, which fixes
 * the chain order of buckets longer than the sorted build handles). The relation is read once
 * (hj3d_partition reads it twice); destination p's pairs go to out_pairs_dev + p * stride pairs
 * (stride >= 1, nparts <= 256; out_pairs_dev holds nparts * stride pairs), counts_dev[p] (device
 * u64) = the number of tuples destined to p. Pairs past a destination's stride are NOT written
 * (a spill): when any counts_dev[p] > stride the caller re-partitions with hj3d_partition (the
 * counts are the same). hj3d_partition_stride gives a bounded stride that distinct keys spill with
 * negligible probability (mean + max(8 sigma of the binomial destination count, mean / 64) + 2
 * tiles; the mean / 64 covers keys repeated ~10 times, as config D's S.a), so the send
 * buffer is ~|rel| pairs instead of nparts x |rel| (stride = rel->n never spills). preds / npred:
 * an optional selection as in hj3d_partition_sel (npred = 0: none). Send it with
 * hj3d_comm_exchange_strided (same stride). Replaces the same seam as hj3d_partition
 * (the reference itself runs on one node, main_experiment1.cc:623-848). */
hj3d_status hj3d_partition_strided(hj3d_ctx* ctx, const hj3d_rel* rel, const hj3d_sel_pred* preds, uint32_t npred,
                                   uint64_t num_buckets, uint32_t nparts, void* out_pairs_dev, uint64_t stride,
                                   void* counts_dev);
uint64_t hj3d_partition_stride(uint64_t n, uint32_t nparts);
/* Owned bucket range of part p: [lo, hi) with lo = ceil(p*NB/nparts). */
void hj3d_part_range(uint64_t num_buckets, uint32_t nparts, uint32_t part, uint64_t* lo, uint64_t* hi);
/* Slice geometry the packed unique probe takes for a chaining table of nb_local buckets holding
 * n_build entries (diagnostic; no device work): out = {W, P, C, W1, P1}: P slices of W buckets
 * (one slice's directory + entries fill one probe workgroup's LDS); C > 1: two partition levels,
 * P1 coarse ranges of W1 = C * W buckets. Replaces nothing of the reference (whose chains are not
 * partitioned); bench.py reports it beside config D's line. */
hj3d_status hj3d_probe_geometry(hj3d_ctx* ctx, uint64_t nb_local, uint64_t n_build, uint32_t out[5]);

/* ---- the exchange itself: RCCL over xGMI, one communicator per context ----
 * One process (or host thread) per GPU, one context per process. RCCL is resolved at run time: a
 * librccl already mapped into the process (torch's) is used, else /opt/rocm's (hj3d_runtime_info
 * names the files). Collective calls must be made by every rank in the same order.
 *   hj3d_comm_unique_id  rank 0 creates the 128-byte communicator id; the host hands it to the
 *                        other ranks by any side channel (torch.distributed broadcast, a file, MPI);
 *   hj3d_comm_init       every rank joins (synchronous; collective);
 *   hj3d_comm_counts     all-to-all of per-destination counts of `chunks` partitioned chunks at once:
 *                        counts_dev = device i64 [chunks][world] (the counts hj3d_partition wrote,
 *                        one row per chunk); send_host / recv_host = host i64 [chunks][world],
 *                        recv[c][p] = elements rank p sends this rank in chunk c (synchronous: the
 *                        one host synchronisation of an exchange strand; collective);
 *   hj3d_comm_counts_cap the same, with this rank's receive capacity (elements it can take over
 *                        the chunks): the ranks agree by an all-reduce whether any rank's total
 *                        exceeds its capacity, and then EVERY rank returns HJ3D_EOVERFLOW, before
 *                        any pair collective (recv_cap = UINT64_MAX: hj3d_comm_counts);
 *   hj3d_comm_exchange   grouped send / recv of one chunk: send_dev holds send_counts[p] elements of
 *                        elem_bytes for every peer p back to back (hj3d_partition's layout), recv_dev
 *                        receives recv_counts[p] elements from every peer in rank order. A receive
 *                        total above recv_cap returns HJ3D_EOVERFLOW BEFORE the collective: every
 *                        rank knows its totals from hj3d_comm_counts, so size recv_dev from them
 *                        (a rank that skips the call leaves its peers waiting; hj3d_comm_counts_cap
 *                        makes that refusal collective). ticket == NULL:
 *                        enqueued on the context stream. ticket != NULL: enqueued on the context's
 *                        exchange stream after the work already on the context stream, so probes of
 *                        earlier chunks overlap it; hj3d_comm_wait(ticket) orders the context stream
 *                        after it (tickets count up; a ticket older than the 64 latest waits for a
 *                        later exchange of the same stream, never too early). Collective;
 *   hj3d_comm_allreduce_u64 / hj3d_comm_allgather  merge the per-rank result slots and statistics
 *                        (u64 counters add, extremes max / min; xor via all-gather), on the context
 *                        stream. Collective. */
#define HJ3D_COMM_ID_BYTES 128
enum { HJ3D_RED_SUM = 0, HJ3D_RED_MAX = 1, HJ3D_RED_MIN = 2 };
hj3d_status hj3d_comm_unique_id(hj3d_ctx* ctx, uint8_t* id);
hj3d_status hj3d_comm_init(hj3d_ctx* ctx, const uint8_t* id, int rank, int world);
hj3d_status hj3d_comm_destroy(hj3d_ctx* ctx);
hj3d_status hj3d_comm_rank(const hj3d_ctx* ctx, int* rank, int* world);
hj3d_status hj3d_comm_counts(hj3d_ctx* ctx, const void* counts_dev, uint32_t chunks, int64_t* send_host,
                             int64_t* recv_host);
hj3d_status hj3d_comm_counts_cap(hj3d_ctx* ctx, const void* counts_dev, uint32_t chunks, uint64_t recv_cap,
                                 int64_t* send_host, int64_t* recv_host);
hj3d_status hj3d_comm_exchange(hj3d_ctx* ctx, const void* send_dev, const int64_t* send_counts, void* recv_dev,
                               const int64_t* recv_counts, uint64_t recv_cap, uint32_t elem_bytes,
                               uint32_t* ticket);
/* The same with peer p's elements at send_dev + p * send_stride elements (hj3d_partition_strided's
 * layout; send_stride = 0: back to back); a send count above send_stride is HJ3D_EINVAL.
 * MANDATORY before this call on every rank: check the partitioner's counts against the stride and
 * re-partition a spilled chunk (hj3d_partition_strided above). The EINVAL is local to the rank
 * that spilled; its peers, already inside the collective, would wait for it forever. */
hj3d_status hj3d_comm_exchange_strided(hj3d_ctx* ctx, const void* send_dev, uint64_t send_stride,
                                       const int64_t* send_counts, void* recv_dev, const int64_t* recv_counts,
                                       uint64_t recv_cap, uint32_t elem_bytes, uint32_t* ticket);
hj3d_status hj3d_comm_wait(hj3d_ctx* ctx, uint32_t ticket);
hj3d_status hj3d_comm_allreduce_u64(hj3d_ctx* ctx, void* buf_dev, uint64_t n, int op);
hj3d_status hj3d_comm_allgather(hj3d_ctx* ctx, const void* send_dev, void* recv_dev, uint64_t bytes);
/* Which HIP runtime (and RCCL) this library runs on: file names and versions, as text. hj3d_ctx_create
 * fails with HJ3D_EDEVICE (reason on stderr) when two HIP runtimes are mapped into the process. */
hj3d_status hj3d_runtime_info(char* buf, uint64_t cap);

/* ---- #dv pre-pass (the number of distinct join-attribute values sizes the build-on-S.a plans:
 * NB = #dv(S.a) / b, main_experiment1.cc:453-454 counts it with an unordered_set, 875, 1001,
 * 1214 use it). One GPU: key_bitmap + or_popcount with rows = 1. Multi-GPU (SURVEY §8e step 1,
 * hj3d/dist.py num_distinct): each rank builds the bitmap of its slice, the ranks all-to-all
 * the bitmap in nranks equal slices, each ORs the slices it received (rows = nranks) and
 * popcounts, and the counts are summed. ----
 * hj3d_key_bitmap: sets bit k of bitmap_dev (u32 words, ceil(domain / 32) of them, zeroed by the
 * caller) for every key k < domain of rel; outside_dev (u64, may be NULL) += #keys >= domain. */
hj3d_status hj3d_key_bitmap(hj3d_ctx* ctx, const hj3d_rel* rel, uint64_t domain, void* bitmap_dev,
                            void* outside_dev);
/* count_dev (u64) += popcount of the OR of `rows` bitmaps of `words` u32 words each, stored
 * back to back at bitmaps_dev. */
hj3d_status hj3d_bitmap_or_popcount(hj3d_ctx* ctx, const void* bitmaps_dev, uint32_t rows, uint64_t words,
                                    void* count_dev);

/* ---- measurement: the box's streaming-copy peak, measured in the same run as the
 * kernels whose roofline fractions are quoted. Replaces nothing of the reference. ----
 * Synchronous: copies `bytes` (a multiple of 16) from src_dev to dst_dev `reps` times for each of
 * six variants (plain / non-temporal 16-B vectors, 4 / 8 / 16 workgroups per CU), each launch timed
 * by HIP events on the context stream; out[0] = the best rate in GB/s (read + write bytes), out[1] =
 * the median launch of that variant, out[2] = its id (workgroups per CU, + 100 when non-temporal). */
hj3d_status hj3d_stream_copy(hj3d_ctx* ctx, void* dst_dev, const void* src_dev, uint64_t bytes, uint32_t reps,
                             double out[3]);

/* ---- selection pushdown: AlgSelection / AlgDynSelection (algebra.hh:278-358) on the device ----
 * The predicate is a conjunction of `npred` (<= HJ3D_SEL_MAX) comparisons of one u32 tuple word
 * (byte offset word_off, compared as int32 when is_signed, else as uint32) against lo (and hi for
 * HJ3D_SEL_RANGE: lo <= v < hi). The passing tuples of `rel` are written, in scan order, to
 * out_pairs_dev as {u32 key, u32 row} (row = the tuple's row id in rel, capacity rel->n pairs);
 * count_dev (device u64) receives their number. The pairs are a relation {out, n, stride 8,
 * key_off 0, row_off 4} that hj3d_build / hj3d_probe take as the selection's consumer would:
 * same order, same row identities. Asynchronous. */
#define HJ3D_SEL_MAX 4
enum { HJ3D_SEL_LT = 0, HJ3D_SEL_LE, HJ3D_SEL_GT, HJ3D_SEL_GE, HJ3D_SEL_EQ, HJ3D_SEL_NE, HJ3D_SEL_RANGE };
struct hj3d_sel_pred {
  uint32_t word_off;  /* byte offset of the compared u32 word, multiple of 4, < stride */
  uint32_t op;        /* HJ3D_SEL_*                                                    */
  uint32_t is_signed; /* compare as int32 (the reference's attrval_t is int)           */
  uint32_t reserved;
  int64_t lo, hi;
};
hj3d_status hj3d_select(hj3d_ctx* ctx, const hj3d_rel* rel, const hj3d_sel_pred* preds, uint32_t npred,
                        void* out_pairs_dev, void* count_dev);
/* Probe strand behind a selection: scan(probe) -> AlgSelection -> probe, as hj3d_probe of the
 * passing tuples (rows = their rows in `probe`). On the partitioned probe path (chaining or nested
 * table) with one predicate the selection is fused into the probe-side partitioner (the failing tuples are
 * dropped where the tuples are read; no extra pass); otherwise hj3d_select runs first
 * (synchronous count read). Result: n_probe = passing tuples (the selection's count()), the
 * other fields as hj3d_probe. Dense output (chaining + HJ3D_PROBE_UNIQUE) fills n_probe slots
 * and needs out_cap >= probe->n. */
hj3d_status hj3d_probe_sel(hj3d_ctx* ctx, const hj3d_table* t, const hj3d_rel* probe, const hj3d_sel_pred* preds,
                           uint32_t npred, uint32_t flags, void* out_dev, uint64_t out_cap);

/* ---- selection over stored nested tuples ----
 * hj3d_select_nested replaces AlgSelection / AlgDynSelection::step (algebra.hh:278-358) stacked on an
 * AlgNestJoinProbe (algebra.hh:435-459), i.e. a selection between the nested probe and the unnest
 * (main_algebra_example.cc:226-234, 305-316): it forwards, in scan order, the stored nested tuples whose
 * predicate holds. A predicate compares one u32 taken from the tuple's base row, from the size of one
 * of its groups, or from the first build tuple of one of its groups (the reference reads both through
 * MainNode). */
/* where a nested-tuple predicate takes the u32 it compares */
enum { HJ3D_NSEL_BASE = 0,   /* word at pred.word_off of the base tuple whose row id is a          */
       HJ3D_NSEL_COUNT = 1,  /* |G_slot|: sub_len of main record ref_slot of tables[slot - 1]     */
       HJ3D_NSEL_FIRST = 2 };/* word at pred.word_off of the tuple of builds[slot - 1] whose row is
                                that main record's first build row (MainNode::data())             */
typedef struct {
  uint32_t source;      /* HJ3D_NSEL_*                                   */
  uint32_t slot;        /* COUNT / FIRST: 1..k; BASE: 0                  */
  hj3d_sel_pred pred;   /* op, is_signed, lo, hi as hj3d_select; word_off unused (0) for COUNT */
} hj3d_nsel_pred;
/* nested_dev: n stored nested tuples {u32 a, u32 ref_1 .. ref_k} of k + 1 words (4-byte aligned),
 * 0 <= k <= HJ3D_NEST_MAX: every width the family produces ({a}, a HJ3D_PROBE_MAINREF probe's dense
 * output as it stands, hj3d_probe_refn's output of up to 7 words). base (the relation a is a row of),
 * tables (k entries, ref_i a main ref of tables[i - 1]) and builds (k entries, builds[i - 1] the relation
 * tables[i - 1] was built from) may be NULL, and so may an entry of tables; an entry of builds with
 * stride 0 counts as not given. A predicate whose source object is missing (BASE without base, COUNT
 * without its table, FIRST without its table or build relation) is HJ3D_EINVAL.
 * A tuple is dead iff base is given and a is not a row of it (implicit rows: tuple index
 * a - base->row_base), or any ref is 0xFFFFFFFF, or a ref whose table is given is not below that table's
 * current main-record count (the rule of hj3d_unnest), or a FIRST predicate's first build row is not a
 * row of its build relation. Dead tuples are dropped, as AlgNestJoinProbe passes nothing downstream
 * without a match; no memory is read through a dead tuple. A ref whose table is not given is opaque:
 * compared with 0xFFFFFFFF and copied. With npred == 0 the operator is this compaction alone.
 * The predicate is the conjunction of npred <= HJ3D_SEL_MAX predicates, each evaluated as hj3d_select
 * evaluates its own (int32 or uint32 compare of the source word against lo, or lo <= v < hi); COUNT
 * compares the u32 sub_len. Each embedded hj3d_sel_pred must be valid for its relation (word_off a
 * multiple of 4 inside the tuple, a known op).
 * With HJ3D_PROBE_EMIT the passing tuples are written unchanged, k + 1 words each, IN INPUT ORDER
 * (AlgSelection forwards in scan order, algebra.hh:295-300; hj3d_select is stable too), at most out_cap
 * of them: when more pass, the first out_cap passing tuples are the ones written. Nothing is written at
 * or beyond out_dev + 4 (k + 1) out_cap. nested_dev and out_dev must not overlap.
 * Result (the probe result slot, hj3d_probe_result): n_probe = n, n_matched = live tuples, n_out =
 * passing tuples, n_cmps = 0, sum_a = the sum of a over the passing tuples (always); with
 * HJ3D_PROBE_CHECKSUM sum_h / xor_h fold h = mix64(a) for k = 0, else h = pair(a, ref_1), then
 * h = mix64(h ^ ref_i) for i = 2..k (else 0); sum_b = sum_c = 0. HJ3D_EOVERFLOW (complete counters) if
 * n_out > out_cap under EMIT.
 * flags: HJ3D_PROBE_EMIT and HJ3D_PROBE_CHECKSUM only. HJ3D_EINVAL: any other flag, a null ctx, k above
 * HJ3D_NEST_MAX, npred above HJ3D_SEL_MAX (or npred && !preds), a slot outside 1..k (BASE: not 0), an
 * unknown source or op, a chaining table, an invalid base or build relation or one with explicit rows,
 * nested_dev or out_dev not 4-byte aligned, n && !nested_dev, EMIT with out_dev == NULL and out_cap > 0,
 * n >= 2^32. Asynchronous on the context stream; pending nested builds of the given tables are finished
 * first, as by a probe. */
hj3d_status hj3d_select_nested(hj3d_ctx* ctx, const void* nested_dev, uint64_t n, uint32_t k,
                               const hj3d_rel* base, const hj3d_table* const* tables, const hj3d_rel* builds,
                               const hj3d_nsel_pred* preds, uint32_t npred,
                               uint32_t flags, void* out_dev, uint64_t out_cap);

/* ---- aggregation over stored nested tuples without unnesting ----
 * The reference has no aggregation operator: a plan that wants COUNT(*), SUM(s.b) or MIN(t.b) per probe
 * tuple, or over the whole join, runs its unnest functors (AlgUnnestHt::step, algebra.hh:490-541) and
 * reduces their output. The nested representation already holds what these aggregates need: with G_i the
 * group ref_i names, the aggregates over the rows a tuple {a, ref_1 .. ref_k} would unnest to are
 *   COUNT = prod |G_j|,  SUM(builds[i].w) = (sum of w over G_i) * prod_{j != i} |G_j|,
 *   MIN / MAX(builds[i].w) = min / max of w over G_i,
 * so no output row is needed. hj3d_group_agg reduces a build word per group (it depends on the table and
 * the build column only and is reused by any number of probes and plans); hj3d_agg_nested combines. */
/* One record of hj3d_group_agg's column, indexed by main ref. */
typedef struct { uint64_t sum, min, max; } hj3d_gagg;
/* hj3d_group_agg: for every main record m of the nested table t, fold the u32 at word_off of the tuple
 * row - build->row_base of `build` (implicit rows) over the rows of m's group, sign-extended (is_signed)
 * or zero-extended to 64 bits: out_dev[m] = {sum, min, max}, sum exact in two's complement (fewer than
 * 2^32 rows, each below 2^32 in magnitude: no overflow), min / max the extended values (as int64 /
 * uint64). A row that is not a row of `build` (the caller passed another relation than the one the table
 * was built from) is skipped and no memory is read through it; a group with no folded row gets the
 * identities: sum 0, min = INT64_MAX / UINT64_MAX, max = INT64_MIN / 0 (signed / unsigned).
 * Result (the probe result slot, hj3d_probe_result): n_probe = main records, n_matched = groups all of
 * whose rows were folded, n_out = rows folded, sum_a = the sum of all sum fields mod 2^64, the rest 0.
 * HJ3D_EOVERFLOW if out_cap is below the table's main-record count (known on the host once a pending
 * build is finished, which the call does first, as a probe does); nothing is written then. HJ3D_EINVAL: a
 * null ctx / t / build, a chaining table, an invalid build relation or one with explicit rows, word_off
 * not a multiple of 4 or not inside the tuple, out_dev not 8-byte aligned, out_dev == NULL with a
 * non-empty table. A cleared table writes nothing and reports zeros. The column is valid as long as main
 * refs are: until the table's next hj3d_build, hj3d_build_many or hj3d_table_clear. Otherwise
 * asynchronous on the context stream. */
hj3d_status hj3d_group_agg(hj3d_ctx* ctx, const hj3d_table* t, const hj3d_rel* build, uint32_t word_off,
                           uint32_t is_signed, void* out_dev, uint64_t out_cap);

#define HJ3D_AGG_MAX 8 /* aggregates one hj3d_agg_nested call computes */
enum { HJ3D_AGG_COUNT = 0, HJ3D_AGG_SUM, HJ3D_AGG_MIN, HJ3D_AGG_MAX_ };
typedef struct {
  uint32_t op, slot;            /* HJ3D_AGG_*; slot 1..k: the group aggregated; COUNT: 0               */
  uint32_t is_signed, reserved; /* MIN / MAX compare as int64 or uint64 (as the column was built)      */
  const void* gcol;             /* hj3d_gagg column of tables[slot - 1] (device, 8-byte aligned); COUNT: NULL */
  uint64_t gcol_n;              /* its records; must be >= that table's main-record count              */
} hj3d_agg_spec;
typedef struct { uint64_t n_in, n_live, c_top; uint64_t total[HJ3D_AGG_MAX]; } hj3d_aggn_res;
/* hj3d_agg_nested: nested_dev holds n tuples {u32 a, u32 ref_1 .. ref_k} (4-byte aligned), ref_i a main ref
 * of tables[i - 1], 1 <= k <= HJ3D_NEST_MAX. Liveness is hj3d_unnestn's: a tuple with any ref not below its
 * table's current main-record count is dead and nothing is read through it. Per tuple and spec, over the
 * rows the tuple would unnest to, with P = prod |G_j|: COUNT = P; SUM = gcol[ref_slot].sum * (P / |G_slot|),
 * computed as the product of the other lengths in u64 arithmetic mod 2^64 (the engine's sum_* counters
 * wrap the same way); MIN / MAX = gcol[ref_slot].min / .max. A dead tuple gives COUNT 0, SUM 0 and MIN / MAX
 * the identities of hj3d_group_agg.
 * With HJ3D_PROBE_EMIT row i of out_dev holds the nspec u64 values of input tuple i (dense, input order: a
 * column aligned with the nested tuples), at most out_cap rows; nothing is written at or beyond
 * out_dev + 8 nspec out_cap. hj3d_agg_nested_result returns HJ3D_EOVERFLOW (with the complete totals) when
 * n > out_cap under EMIT. total[s] = the sum mod 2^64 of spec s's values (COUNT, SUM), or their min / max
 * over the live tuples (the identity if there are none); c_top = the sum of P = hj3d_unnestn's c_top.
 * The magnitude rule is hj3d_unnestn's: a tuple's P, or c_top, at or beyond 2^63 makes
 * hj3d_agg_nested_result return HJ3D_EUNSUPPORTED with only n_in and n_live set.
 * flags: HJ3D_PROBE_EMIT only. HJ3D_EINVAL: any other flag, a null ctx / tables / entry of tables, a chaining
 * table, k outside 1 .. HJ3D_NEST_MAX, nspec outside 1 .. HJ3D_AGG_MAX (or a null specs), an unknown op, a
 * slot outside 1 .. k (COUNT: not 0), a null gcol where one is needed, gcol_n below the table's main-record
 * count, nested_dev not 4-byte or out_dev / gcol not 8-byte aligned, n && !nested_dev, EMIT with
 * out_dev == NULL and out_cap > 0, n >= 2^32; hj3d_agg_nested_result before any hj3d_agg_nested. The result
 * has a slot of its own: the probe and hj3d_unnestn result slots are not touched. Asynchronous; pending
 * nested builds of the given tables are finished first, as by a probe. */
hj3d_status hj3d_agg_nested(hj3d_ctx* ctx, const void* nested_dev, uint64_t n, uint32_t k,
                            const hj3d_table* const* tables, const hj3d_agg_spec* specs, uint32_t nspec,
                            uint32_t flags, void* out_dev, uint64_t out_cap);
hj3d_status hj3d_agg_nested_result(hj3d_ctx* ctx, hj3d_aggn_res* out);

/* ---- the same aggregates per build key: join + GROUP BY a build key ----
 * SELECT s.key, COUNT(*), SUM(r.x), MIN(t.y) FROM R join S join T GROUP BY s.key. The main ref of the by-table
 * is the group id, so the aggregates are reduced into a column indexed by that main ref: the column shape
 * hj3d_group_agg produces and hj3d_agg_nested consumes. */
typedef struct {
  uint32_t op, slot;  /* HJ3D_AGG_*; slot 1..k: a group's hj3d_gagg column; slot 0: COUNT, or (op != COUNT) a word
                         of the base row                                                                        */
  uint32_t is_signed; /* MIN / MAX order, and the extension of a base word                                      */
  uint32_t word_off;  /* slot 0, op != COUNT: byte offset of the u32 in the base tuple; else 0                   */
  const void* gcol;   /* slot >= 1: hj3d_gagg column of tables[slot - 1] (device, 8-byte aligned); else NULL     */
  uint64_t gcol_n;    /* its records; must be >= that table's main-record count                                 */
} hj3d_gby_spec;
/* hj3d_agg_grouped: nested_dev holds n tuples {u32 a, u32 ref_1 .. ref_k} exactly as for hj3d_agg_nested, and
 * liveness is hj3d_agg_nested's: a tuple with any ref not below its table's main-record count is dead. If any
 * spec has slot 0 with op != COUNT, `base` is required (implicit rows) and a tuple whose a is not a row of
 * base (a - row_base outside [0, n)) is dead too, hj3d_select_nested's rule; without such a spec base may be
 * NULL and a is opaque. Nothing is read through a dead tuple.
 * Per tuple and spec, with P = prod |G_j|: for slot >= 1 and for COUNT exactly the value hj3d_agg_nested
 * defines; for a base-word spec SUM = ext(w) * P mod 2^64 and MIN / MAX = ext(w), w the u32 at word_off of base
 * row a, sign- (is_signed) or zero-extended to 64 bits.
 * out_dev is a column of n_mains(tables[by_slot - 1]) rows of nspec u64 (8-byte aligned): row m, field s = the
 * sum mod 2^64 (COUNT, SUM), or the min / max in the spec's order, of spec s's values over the live tuples with
 * ref_by_slot == m; a group without a live tuple gets 0 / 0 / the identities of hj3d_group_agg. The operator
 * initialises the column itself. out_cap (rows) below the main-record count gives HJ3D_EOVERFLOW and nothing is
 * written (hj3d_group_agg's rule); nothing is ever written at or beyond out_dev + 8 nspec out_cap.
 * flags: HJ3D_PROBE_ACCUMULATE only. With it the column is not initialised and the call folds into what is
 * there (a strand issued in chunks, several inputs grouped into one column); the result slot restarts on every
 * call either way.
 * hj3d_agg_grouped_result: n_in, n_live, c_top and total[s] as hj3d_agg_nested defines them over this call's
 * tuples, so total[s] is the reduce of column s over all groups (without ACCUMULATE). The magnitude rule is
 * hj3d_agg_nested's: a P, or c_top, at or beyond 2^63 gives HJ3D_EUNSUPPORTED with only n_in and n_live set,
 * and the column is then unspecified. The result has a slot of its own: the probe, hj3d_unnestn and
 * hj3d_agg_nested result slots are not touched.
 * HJ3D_EINVAL: any other flag; a null ctx / tables / entry of tables / specs; a chaining table; k outside
 * 1 .. HJ3D_NEST_MAX; by_slot outside 1 .. k; nspec outside 1 .. HJ3D_AGG_MAX; an unknown op; slot > k; COUNT with
 * slot != 0; slot >= 1 with a null gcol or gcol_n below that table's main-record count; slot 0 with op != COUNT
 * and base null, invalid or with explicit rows, or word_off not a multiple of 4 or outside the tuple;
 * nested_dev not 4-byte or out_dev / gcol not 8-byte aligned; n && !nested_dev; out_dev == NULL with a
 * non-empty by-table; n >= 2^32; hj3d_agg_grouped_result before any hj3d_agg_grouped.
 * Asynchronous on the context stream; pending nested builds of the given tables are finished first, as by a
 * probe. A cleared by-table writes nothing and reports n_live = 0. HJ3D_OPT_GBY_FORM picks the kernel form;
 * every form gives the same column. */
hj3d_status hj3d_agg_grouped(hj3d_ctx* ctx, const void* nested_dev, uint64_t n, uint32_t k,
                             const hj3d_table* const* tables, uint32_t by_slot, const hj3d_rel* base,
                             const hj3d_gby_spec* specs, uint32_t nspec, uint32_t flags, void* out_dev,
                             uint64_t out_cap);
hj3d_status hj3d_agg_grouped_result(hj3d_ctx* ctx, hj3d_aggn_res* out);

/* ---- synthetic key/FK relations generated on the device (bench / full-size checks) ----
 * R.k = a seeded bijective permutation of [0, n_keys) (keys for global rows
 * [row_base, row_base+n)), written into tuple word key_off of an AoS buffer;
 * S.a = uniform in [0, fk_max) from a counter-based RNG of the global row id. */
hj3d_status hj3d_gen_keys(hj3d_ctx* ctx, void* tuples_dev, uint64_t n, uint32_t stride, uint32_t key_off,
                          uint64_t row_base, uint64_t n_keys, uint64_t seed);
hj3d_status hj3d_gen_fk(hj3d_ctx* ctx, void* tuples_dev, uint64_t n, uint32_t stride, uint32_t key_off,
                        uint64_t row_base, uint32_t fk_max, uint64_t seed);
/* S.a ~ Zipf(theta) over [0, fk_max) (value 0 the most frequent; P(v) ~ (v+1)^-theta), sampled by
 * rejection-inversion (the method of util/zipf_distribution.hh) from a counter-based RNG of the
 * global row id: config C (nested table, Zipf 0.8 duplicates) at full size. */
hj3d_status hj3d_gen_zipf(hj3d_ctx* ctx, void* tuples_dev, uint64_t n, uint32_t stride, uint32_t key_off,
                          uint64_t row_base, uint32_t fk_max, double theta, uint64_t seed);
/* ---- the reference's own input generators (host, synchronous, bit-exact) ----
 * hj3d_gen_exp1_ref replaces Experiment1::init (main_experiment1.cc:415-457): one std::mt19937
 * stream (seed 5489) shuffles R.k = iota(nR) (std::shuffle), draws S.a uniform over [0, fkMax)
 * (GenRandIntVec::generate_uni, util/GenRandIntVec.cc:72-98) or Zipf(theta) - 1
 * (generate_zipf :167-200, util/zipf_distribution.hh:48-58), then permutes S.a (vec_permute
 * :335-340); fkMax = nR >> t (main_experiment1.cc:190). Writes the columns Rk[nR], Sa[nS] to
 * HOST memory; S.k is the row id. theta: the reference's experiment 1 fixes 1.0 (:444); config C
 * uses 0.8. threads: workers for the Zipf attempts (0 = min(hardware threads, 16)); the result does
 * not depend on it.
 * hj3d_gen_exp4_ref replaces Experiment4::init (main_experiment4.cc:517-575): S.a, T.a of
 * card = (2^log2R >> alpha) * mult_a + (2^log2R >> beta) * mult_b tuples each (R.k, S.k, T.k =
 * iota). With Sa or Ta NULL only *card is written. */
hj3d_status hj3d_gen_exp1_ref(uint64_t nR, uint64_t nS, int skew, double theta, uint32_t t, uint32_t* Rk,
                              uint32_t* Sa, int threads);
hj3d_status hj3d_gen_exp4_ref(uint32_t log2R, uint32_t alpha, uint32_t mult_a, uint32_t beta, uint32_t mult_b,
                              uint32_t* Sa, uint32_t* Ta, uint64_t* card);
/* Expected key/FK join aggregates WITHOUT a hash table (full-size verification of the
 * key/FK plans): `build` holds unique keys in [0, n_keys); every probe tuple's partner row is
 * inv[key], inv being the inverse of the build key column. Probe keys outside [0, n_keys) are
 * skipped, and keys of the domain that no build row holds join with nothing (a build side may
 * cover only part of the domain: a rank's shard, an R shorter than n_keys); build row id
 * 0xFFFFFFFF is reserved (it marks "no row" in inv). Accumulates {n_out, sum_a, sum_b,
 * sum_h, xor_h} (u64 each) into res_dev (zero it first). Orientation: a = probe row,
 * b = build row; with swap != 0, a = build row, b = probe row (plans that build on the FK side). */
hj3d_status hj3d_expected_fk_join(hj3d_ctx* ctx, const hj3d_rel* build, const hj3d_rel* probe, uint64_t n_keys,
                                  int swap, void* res_dev);
/* The same expectation when the build keys were made by hj3d_gen_keys(n_keys, key_seed): the
 * partner row of key k is the inverse permutation of k (per-rank verification on multi-GPU). */
hj3d_status hj3d_expected_fk_join_gen(hj3d_ctx* ctx, const hj3d_rel* probe, uint64_t n_keys, uint64_t key_seed,
                                      int swap, void* res_dev);

#ifdef __cplusplus
}
#endif
#endif /* HJ3D_H */
