/*
 * emqx_tm.h -- C ABI of the MI355X topic-matching engine (libemqx_tm.so).
 *
 * Drop-in boundary for EMQ X's publish-time matching path.  The reference is
 * pure Erlang and has no FFI of its own; each entry point below names the
 * reference function it replaces (paths relative to the reference tree).  An
 * erl_nif shim (emqx_amd/csrc/nif/emqx_tm_nif.c) binds these
 * 1:1 to the Erlang module API.
 *
 * Conventions
 *   - plain pointers + sizes; caller-owned inputs are borrowed for the call;
 *   - return codes: 0 = ok, negative errno-style values (TM_E*) on error;
 *     predicates return 0/1; no C++ exceptions cross this boundary;
 *   - one engine = one host trie mirrored into one HBM replica per device it
 *     was created on (tm_create: one device; tm_create_replicated: a list).
 *     Calls on one engine are serialised by an internal mutex (readers and the
 *     single writer of the reference's mnesia tables become ordered operations
 *     on each replica's HIP stream, so a match issued after tm_trie_insert
 *     returns always sees the filter on every device: read-your-writes,
 *     src/emqx_broker.erl:150-158).
 */
#ifndef EMQX_TM_H
#define EMQX_TM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TM_OK          0
#define TM_ENOENT     (-2)
#define TM_EIO        (-5)
#define TM_ENOMEM     (-12)
#define TM_ENODEV     (-19)
#define TM_EINVAL     (-22)
#define TM_EOVERFLOW  (-75)
#define TM_EABORT     (-125)   /* mnesia:abort({node_not_found, _}), src/emqx_trie.erl:203 */

#if defined(__GNUC__)
#define TM_API __attribute__((visibility("default")))
#else
#define TM_API
#endif

#define TM_NONE        0xFFFFFFFFu
#define TM_MAX_TOPIC_LEN 4096  /* ?MAX_TOPIC_LEN, src/emqx_topic.erl:45 */

typedef struct tm_engine tm_engine;
typedef struct tm_batch  tm_batch;

typedef struct {
    int32_t  device;        /* HIP device ordinal; -1 = host-only engine (trie ops, no match) */
    uint32_t init_slots;    /* initial edge-hash capacity in 32-B slots (0 = default) */
    uint32_t host_threads;  /* threads for host tokenise+intern (0 = auto) */
    uint32_t flags;         /* TM_CFG_* bits; unknown bits are rejected */
} tm_config;

/* Filter-sharded mode: the word dictionary is shared by every shard engine and
 * grows only through tm_dict_load (called identically on every shard), so the
 * u32 word ids of a tokenised topic mean the same on every GPU and tokenised
 * publish batches can be exchanged between devices.  tm_trie_insert of a filter
 * with a word outside the dictionary fails with TM_ENOENT. */
#define TM_CFG_FROZEN_DICT 1u
/* Tokenise + intern publish batches on the host (emqx_topic:words/1 on the
 * CPU, then the word ids are copied to HBM) instead of the default device
 * tokeniser, which copies the topic bytes and tokenises them in HBM against
 * the device mirror of the word dictionary.  Results are identical. */
#define TM_CFG_HOST_TOKENIZE 2u

/* #trie_node{} view (include/emqx.hrl:98-103) */
typedef struct {
    uint32_t edge_count;
    uint32_t has_topic;     /* topic =/= undefined */
    uint32_t filter_id;     /* id of `topic` when has_topic, else TM_NONE */
} tm_trie_node;

/* CSR result: row i = sorted (Erlang binary order), deduplicated filter ids
 * matching topic i.  Memory is engine-owned, valid until the next match call on
 * the same engine (or tm_batch_free for batch results). */
typedef struct {
    uint32_t        n_topics;
    uint64_t        n_matches;
    const uint32_t* row_offsets;  /* n_topics + 1 entries */
    const uint32_t* filter_ids;   /* n_matches entries */
} tm_result;

typedef struct {
    uint64_t topics;        /* topics matched */
    uint64_t visits;        /* V: match_node invocations (src/emqx_trie.erl:165-177) */
    uint64_t hash_hits;     /* H: 'match_#' hits (src/emqx_trie.erl:181-186) */
    uint64_t words;         /* sum of topic depths d */
    uint64_t matches;       /* sum |M(t)| */
    uint64_t slow_topics;   /* topics served by the generic (deep/irregular/overflow) kernel */
    uint64_t overflow_tiles;
    float    ms_match;      /* device time of the frontier kernel (last launch) */
    float    ms_total;      /* device time of the whole batch pipeline (last launch) */
    float    ms_tokenize;   /* device tokeniser time of the last launch (0: tokens reused) */
    uint64_t probes;        /* 64-B edge-hash bucket reads of the tile walk (hits + misses) */
    float    ms_csr;        /* device time of the last dense-CSR build (scan + copy; 0: not built) */
    float    ms_queue;      /* device time from the last launch call to its pipeline's start (work queued ahead) */
    uint64_t iterations;    /* frontier iterations of the tile walk (each pops <= 64 probes) */
    uint64_t publishes;     /* publishes of the batch (TM_BATCH_DEDUP: >= topics, the rows) */
    uint64_t delivered;     /* sum over the publishes of their rows' lengths (= matches without dedup) */
    float    ms_dedup;      /* device time of the last device dedup pass (0: none) */
    float    ms_expand;     /* device time of the per-publish row expansion (TM_BATCH_DEDUP) */
} tm_batch_stats;

typedef struct {
    uint64_t version;       /* bumped on every trie mutation */
    uint64_t nodes;         /* live trie nodes incl. root */
    uint64_t edges;         /* live edges (ets:info(emqx_trie, size)) */
    uint64_t filters;       /* nodes with topic =/= undefined */
    uint64_t words;         /* interned words */
    uint64_t slots;         /* edge-hash capacity (32-B slots) */
    uint64_t device_bytes;  /* HBM held by the trie replica */
    uint64_t uploads_full;  /* full trie uploads */
    uint64_t uploads_delta; /* incremental delta uploads */
    uint64_t delta_slots;   /* slots written by delta uploads */
    uint64_t graph_launches;   /* batch launches replayed as a captured HIP graph (repeated or fresh deduplicated batches) */
} tm_engine_stats;

/* ---- engine ---------------------------------------------------------- */
TM_API int  tm_create(const tm_config* cfg, tm_engine** out);
/* One engine over several devices (a node's GPUs): every node of the
 * reference cluster holds the whole emqx_trie (src/emqx_trie.erl:53-74), so
 * the engine keeps ONE host trie and an HBM replica of it on each listed
 * device (a device may be listed twice); cfg->device is ignored.  A mutation
 * is made once and its delta uploaded to every replica, so filter ids are the
 * same everywhere.  Per-publish calls (tm_match_async / tm_match_coalesced)
 * are dealt over the replicas; whole-batch calls (tm_match_batch,
 * tm_match_routes_batch, tm_rules_match, tm_acl_check) of 65,536+ publishes are split into
 * one contiguous slice per replica and their results concatenated (no
 * collective); a fresh tm_batch goes to the next replica round-robin, or to
 * the one named by tm_batch_prepare_on.  n_devices = 0: host-only engine. */
TM_API int  tm_create_replicated(const tm_config* cfg, const int32_t* devices, uint32_t n_devices,
                                 tm_engine** out);
/* Number of device replicas (0 for a host-only engine). */
TM_API uint32_t tm_replica_count(tm_engine* e);
/* Starts the async pipeline (tm_match_async) of every replica now instead of
 * at the first call -- a NIF calls it from new/1, which runs on a dirty
 * scheduler, so the first match_async/3 never pays thread and stream setup. */
TM_API int  tm_async_start(tm_engine* e);
TM_API void tm_destroy(tm_engine* e);
TM_API uint64_t tm_version(tm_engine* e);
TM_API int  tm_stats(tm_engine* e, tm_engine_stats* out);
/* Applies pending trie deltas to the device replica (also done implicitly by
 * every match call). */
TM_API int  tm_sync(tm_engine* e);
/* tm_sync without the wait: the pending deltas are gathered now and their
 * upload is queued on every replica's stream, behind the work already there
 * (a walk in flight keeps its snapshot) and ahead of the next launch. */
TM_API int  tm_sync_async(tm_engine* e);

/* ---- emqx_trie (src/emqx_trie.erl) ----------------------------------- */
/* emqx_trie:insert/1 (:81-93): idempotent; add_path/1 (:145-158) semantics.
 * TM_EOVERFLOW + tm_last_error() (here and from every other call that
 * inserts): the edge hash could not be re-packed so that every key lies
 * within 48 buckets of home (see tm_debug_check); the filter is inserted, and
 * batches do not launch until a later insert has restored the bound. */
TM_API int  tm_trie_insert(tm_engine* e, const uint8_t* topic, size_t len);
/* emqx_trie:delete/1 (:107-116) + delete_path/1 (:190-204). */
TM_API int  tm_trie_delete(tm_engine* e, const uint8_t* topic, size_t len);
/* emqx_trie:lookup/1 (:102-104): returns 1 found, 0 not found.  is_root
 * selects the atom `root` node id. */
TM_API int  tm_trie_lookup(tm_engine* e, const uint8_t* node_id, size_t len, int is_root,
                    tm_trie_node* out);
/* emqx_trie:empty/0 (:119-121): 1 if the edge table is empty. */
TM_API int  tm_trie_empty(tm_engine* e);
/* emqx_trie:match/1 (:96-99) for one topic: writes up to cap ids (sorted by
 * filter bytes), *n_out = full count.  Runs on the device. */
TM_API int  tm_trie_match(tm_engine* e, const uint8_t* topic, size_t len,
                   uint32_t* ids, uint32_t cap, uint32_t* n_out);

/* emqx_trie:match/1 for one topic, blocking, for callers on many threads:
 * tm_match_async below plus a futex wait for the caller's own row, so
 * concurrent callers share device batches formed by the engine's launcher
 * (see tm_match_async / tm_coalesce_config for the batching policy and
 * INTEGRATION.md for how it relates to emqx_batch, src/emqx_batch.erl:56-82).
 * Results and errors as tm_trie_match, per caller (len > TM_MAX_TOPIC_LEN ->
 * TM_EINVAL). */
TM_API int  tm_match_coalesced(tm_engine* e, const uint8_t* topic, size_t len,
                               uint32_t* ids, uint32_t cap, uint32_t* n_out);
/* Sets max_batch (0 = keep; default 16384) and linger_us (TM_NONE = keep;
 * default 0: a batch is whatever queued while the pipeline was busy) of the
 * async pipeline below, which tm_match_coalesced rides on; *batches /
 * *requests (may be NULL) = device batches run and requests served so far. */
TM_API int  tm_coalesce_config(tm_engine* e, uint32_t max_batch, uint32_t linger_us,
                               uint64_t* batches, uint64_t* requests);

/* Asynchronous emqx_trie:match/1 for one topic -- the form the NIF uses:
 * the caller (an Erlang process) returns at once and receives its row later
 * (enif_send), so every publishing process can have a match in flight, as
 * every publisher runs match_routes/1 concurrently in the reference
 * (src/emqx_broker.erl:201-210).  Calls are queued; an engine thread forms
 * device batches from the queue (emqx_batch's size + linger policy,
 * src/emqx_batch.erl:49-90) and keeps up to `depth` of them in flight, each on
 * a HIP stream of its own: H2D of the topics, device tokeniser, trie walk,
 * read-back of the rows.  cb(ctx, rc, ids, n) runs once per call on the
 * engine's completion thread: rc 0 and the topic's sorted filter ids
 * (engine memory, valid during the callback only), or a TM_E* code with no
 * ids.  A match submitted after tm_trie_insert returned sees the filter.
 * Returns TM_EINVAL (no callback) for len > TM_MAX_TOPIC_LEN; callbacks must
 * not destroy the engine. */
typedef void (*tm_match_cb)(void* ctx, int rc, const uint32_t* ids, uint32_t n);
TM_API int  tm_match_async(tm_engine* e, const uint8_t* topic, size_t len, tm_match_cb cb, void* ctx);
typedef struct {
    uint64_t batches;       /* device batches completed */
    uint64_t requests;      /* calls completed */
    uint64_t recoveries;    /* batches re-run through the CSR path (capacity misses) */
    uint64_t max_batch;     /* largest batch formed */
    uint32_t depth;         /* batches in flight at most (TM_ASYNC_DEPTH, default 4) */
    uint32_t queued;        /* calls waiting for a batch now */
    double   us_launch;     /* host time forming + enqueueing batches (launcher thread) */
    double   us_wait;       /* completer time blocked on device batches */
    double   us_deliver;    /* completer time running callbacks */
    uint64_t inline_launches; /* batches a submitting caller launched itself (pipeline idle) */
} tm_async_stats;
TM_API int  tm_async_stats_get(tm_engine* e, tm_async_stats* out);

/* ---- batched publish matching: emqx_router:match_routes/1 hot path ---- */
/* (src/emqx_router.erl:127-141 applied to a batch of publishes,
 *  src/emqx_broker.erl:201-210).  topics = concatenated topic bytes,
 *  offsets[n+1] byte offsets.  Result as tm_result above. */
TM_API int  tm_match_batch(tm_engine* e, const uint8_t* topics, const uint64_t* offsets,
                    uint32_t n, tm_result* out);

/* tm_match_batch for consumers that read the ids in place (the NIF turning
 * them into filter binaries through tm_filters_copy_packed): filter id j of
 * the result is ids[j * id_bytes ..] little-endian, id_bytes = 3 while every
 * node id of the engine fits 24 bits (~16.7M trie nodes), else 4.  The ids
 * cross PCIe packed -- 3/4 of the bytes -- and nobody unpacks them.  Rows
 * (row_offsets, u32) as in tm_result; the buffers live until the next call. */
typedef struct {
    uint32_t        n_topics;
    uint32_t        id_bytes;
    uint64_t        n_matches;
    const uint32_t* row_offsets;
    const uint8_t*  ids;
} tm_result_packed;
TM_API int  tm_match_batch_packed(tm_engine* e, const uint8_t* topics, const uint64_t* offsets,
                    uint32_t n, tm_result_packed* out);

/* Split form for pipelining / device-resident benchmarking:
 * prepare = H2D of the topic bytes and offsets (default), or host tokenise +
 *           intern + H2D of the word ids with TM_CFG_HOST_TOKENIZE
 *           (emqx_topic:words/1, src/emqx_topic.erl:158-164);
 * launch  = enqueue the device pipeline (async): with device tokenisation the
 *           first launch tokenises the bytes in HBM against the dictionary
 *           mirror, after the pending deltas; later launches reuse the tokens
 *           unless the dictionary grew in between;
 * wait    = block until done; result = D2H of the CSR.
 * *out must be NULL (a new batch) or a batch of this engine, which is then
 * re-prepared in place: its device and pinned buffers are reused and only
 * grow, so a caller cycling a few batches allocates nothing in steady state. */
TM_API int  tm_batch_prepare(tm_engine* e, const uint8_t* topics, const uint64_t* offsets,
                      uint32_t n, tm_batch** out);
/* tm_batch_prepare with flags.  TM_BATCH_DEDUP: identical topics of the batch
 * are matched once (hot-topic skew, BASELINE config C5); the result then has
 * one row per DISTINCT topic (tm_result.n_topics = distinct count, rows in
 * first-occurrence order) and tm_batch_row_map gives the row of every
 * publish.  With the device tokeniser (the default) the dedup runs on the
 * device at launch, behind the tokeniser, on every fresh pass over the batch
 * (prepare / tm_batch_retokenize): the row count and row_of exist once the
 * batch has been waited, and tm_batch_publish_rows gives every publish its
 * row in HBM. */
#define TM_BATCH_DEDUP 1u
/* TM_BATCH_STREAM: the batch runs on a HIP stream of its own, so launches of
 * different batches overlap on the device (one batch's CSR pass with the
 * next batch's walk); trie updates still reach a launch that follows them
 * (read-your-writes) and wait for the batch's walk before changing the
 * tables.  Every call on the batch stays synchronous for the caller. */
#define TM_BATCH_STREAM 2u
TM_API int  tm_batch_prepare_ex(tm_engine* e, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                                uint32_t flags, tm_batch** out);
/* tm_batch_prepare_ex on replica `replica` (< tm_replica_count) of the engine.
 * A batch stays on the replica it was created on (re-preparing it on another
 * is TM_EINVAL); tm_batch_replica names it. */
TM_API int  tm_batch_prepare_on(tm_engine* e, uint32_t replica, const uint8_t* topics, const uint64_t* offsets,
                                uint32_t n, uint32_t flags, tm_batch** out);
TM_API uint32_t tm_batch_replica(tm_engine* e, tm_batch* b);
/* row_of[i] = result row of publish i (identity for batches without
 * TM_BATCH_DEDUP); *n_rows = number of result rows.  Engine-owned memory,
 * valid until the batch is re-prepared or freed. */
TM_API int  tm_batch_row_map(tm_engine* e, tm_batch* b, const uint32_t** row_of, uint32_t* n_rows);
TM_API int  tm_batch_launch(tm_engine* e, tm_batch* b);
TM_API int  tm_batch_wait(tm_engine* e, tm_batch* b);
TM_API int  tm_batch_result(tm_engine* e, tm_batch* b, tm_result* out);
/* tm_batch_result with the ids packed on the device as in tm_match_batch_packed
 * (3 bytes while node ids fit 24 bits, else 4), into the batch's own pinned
 * buffers: valid until the batch is re-prepared or freed, so concurrent
 * callers on their own batches (the NIF's match_batch) do not share them. */
TM_API int  tm_batch_result_packed(tm_engine* e, tm_batch* b, tm_result_packed* out);
/* Rows rows[0..k) of a waited batch (each < the batch's row count) as a host
 * CSR: n_topics = k, row i = filter_ids[row_offsets[i] .. row_offsets[i+1]),
 * sorted and deduplicated like tm_batch_result's.  Gathered on the device from
 * where the walk wrote them -- no dense CSR, no whole-batch copy: a self-check
 * of a 10M-publish batch reads ~3,000 rows this way.  Batch-owned memory,
 * valid until the next tm_batch_sample, re-prepare or free of the batch.
 * Replaces nothing in the reference (a diagnostic of the device result). */
TM_API int  tm_batch_sample(tm_engine* e, tm_batch* b, const uint32_t* rows, uint32_t k, tm_result* out);
TM_API int  tm_batch_stats_get(tm_engine* e, tm_batch* b, tm_batch_stats* out);
/* A waited batch's result is the rows as the walk wrote them to HBM: row i
 * (one per topic, or per distinct topic with TM_BATCH_DEDUP) is
 * d_ids[d_start[i] .. d_start[i] + d_count[i]), sorted (Erlang binary order)
 * and deduplicated; rows of different topics are not adjacent.  Device
 * pointers of the batch, valid until its next launch or re-prepare; no copy,
 * no extra pass.  *n_matches = sum of the counts. */
TM_API int  tm_batch_rows(tm_engine* e, tm_batch* b, const uint32_t** d_count, const uint64_t** d_start,
                          const uint32_t** d_ids, uint64_t* n_matches);
/* The result per PUBLISH of a waited batch, on the device: publish i's
 * sorted, deduplicated filter ids are d_ids[d_start[i] .. d_start[i] +
 * d_count[i]).  For a TM_BATCH_DEDUP batch deduplicated on the device this is
 * every publish's row (expanded behind the walk: publishes of one topic share
 * the ids), and *n_delivered = the sum of the counts -- the (publish, filter)
 * matches delivered (emqx_broker:publish/1 matches every message,
 * src/emqx_broker.erl:201-210); without TM_BATCH_DEDUP it is tm_batch_rows.
 * TM_EINVAL for a batch deduplicated on the host. */
TM_API int  tm_batch_publish_rows(tm_engine* e, tm_batch* b, const uint32_t** d_count, const uint64_t** d_start,
                                  const uint32_t** d_ids, uint64_t* n_delivered);
/* Device pointers of the batch's dense CSR: row_offsets[n + 1], ids[total]
 * in topic order.  Built from the rows on first request after a launch
 * (scan + one copy, on the batch's stream; tm_batch_result, routes, dispatch
 * and export build it too); valid until the next launch. */
TM_API int  tm_batch_device_csr(tm_engine* e, tm_batch* b, const uint32_t** d_row_offsets,
                         const uint32_t** d_ids, uint64_t* n_matches);
TM_API void tm_batch_free(tm_engine* e, tm_batch* b);
/* Drops the tokens of a device-tokenised batch: its next launch tokenises the
 * resident bytes again -- a never-seen batch's full device pipeline without a
 * new H2D (bench: pipeline_fresh_ms).  TM_EINVAL for host-tokenised batches. */
TM_API int  tm_batch_retokenize(tm_engine* e, tm_batch* b);

/* ---- routes: emqx_router + emqx_broker:aggre/1 on the device ----------- */
/* One route of `topic` to an aggregated destination id chosen by the caller
 * (emqx_broker:aggre/1, src/emqx_broker.erl:250-261: a node() dest aggregates
 * to the node, a shared-subscription dest {Group, Node} to the Group, so the
 * routes {G, n1} and {G, n2} share one id).  emqx_router:do_add_route/2
 * (src/emqx_router.erl:113-124, 229-234): the first route of a topic puts it
 * into the trie (exact topics too, so one walk returns exact + wildcard
 * matches); a repeated (topic, dest) only counts. */
TM_API int  tm_route_add(tm_engine* e, const uint8_t* topic, size_t len, uint32_t dest);
/* do_delete_route/2 (:163-169, 239-247): TM_ENOENT if (topic, dest) has no
 * route; removing the last route of a topic deletes it from the trie. */
TM_API int  tm_route_delete(tm_engine* e, const uint8_t* topic, size_t len, uint32_t dest);

/* Cluster route delta feed: n route-table events applied
 * in order under one engine lock.  The emqx_route bag and the trie tables are
 * mnesia ram_copies replicated to every node (src/emqx_router.erl:77-86,
 * src/emqx_trie.erl:53-74), so a node sees remote route writes as table
 * events ({write, #route{}} / {delete_object, #route{}}); the feed also carries
 * the deletes of cleanup_routes(Node) on nodedown
 * (src/emqx_router_helper.erl:135-141, 173-177) and the
 * {Group, node()} routes of shared subscriptions (src/emqx_shared_sub.erl:
 * 297-313).  ops[i] = TM_ROUTE_WRITE -> tm_route_add(topic i, dests[i]);
 * TM_ROUTE_DELETE -> tm_route_delete, where a missing (topic, dest) is a no-op
 * (mnesia:delete_object of an absent record).  *n_changed (may be NULL) counts
 * the events that changed the table.  Stops at the first other error. */
#define TM_ROUTE_DELETE 0u
#define TM_ROUTE_WRITE  1u
TM_API int  tm_route_apply(tm_engine* e, const uint8_t* topics, const uint64_t* offsets, const uint32_t* dests,
                           const uint8_t* ops, uint32_t n, uint64_t* n_changed);

/* aggre(match_routes(T)) per topic: row i lists (filter id, dest) pairs,
 * filters in Erlang binary order, each filter's dests in first-added order,
 * no (filter, dest) twice.  Engine-owned memory, valid like tm_result. */
typedef struct {
    uint32_t        n_topics;
    uint64_t        n_routes;
    const uint32_t* row_offsets;  /* n_topics + 1 */
    const uint32_t* filter_ids;   /* n_routes */
    const uint32_t* dests;        /* n_routes */
} tm_routes;

/* Device route resolution of a waited batch (its match CSR stays in HBM). */
TM_API int  tm_batch_routes(tm_engine* e, tm_batch* b, tm_routes* out);
/* tm_match_batch + tm_batch_routes in one call (emqx_router:match_routes/1 +
 * emqx_broker:aggre/1 over a batch of publishes). */
TM_API int  tm_match_routes_batch(tm_engine* e, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                                  tm_routes* out);

/* ---- subscribers + fan-out: emqx_broker dispatch on the device --------- */
/* The local node's subscriber bag (?SUBSCRIBER / ?SUBSCRIPTION,
 * src/emqx_broker.erl:145-196), non-shared subscriptions; subscriber ids are
 * the caller's (one per subscriber pid).  node_dest = the aggregated dest id
 * the caller uses for node() in tm_route_add.
 * tm_subscribe: do_subscribe/4 (:150-158); idempotent per (topic, subscriber)
 * (:127-139); the topic's first subscriber adds route (topic, node_dest)
 * (handle_call({subscribe, Topic}), :438-440 -> emqx_router:do_add_route/1).
 * Topics with > 1024 subscribers are sharded into {shard, Topic, I} keys by the
 * reference (src/emqx_broker_helper.erl:82-87): a storage split of the same
 * set, so a topic keeps one run here, in subscription order. */
TM_API int  tm_subscribe(tm_engine* e, const uint8_t* topic, size_t len, uint32_t subscriber, uint32_t node_dest);
/* do_unsubscribe/4 (:179-191): TM_ENOENT if not subscribed (unsubscribe/1's
 * `[] -> ok`, :170-177); the last subscriber of a topic deletes its route
 * (handle_cast({unsubscribed, Topic}), :463-469). */
TM_API int  tm_unsubscribe(tm_engine* e, const uint8_t* topic, size_t len, uint32_t subscriber, uint32_t node_dest);
/* subscriber_down/1 (:332-347): drops every subscription of the subscriber;
 * *n_removed (may be NULL) = how many. */
TM_API int  tm_subscriber_down(tm_engine* e, uint32_t subscriber, uint32_t node_dest, uint64_t* n_removed);

/* The ?SUBOPTION table: {SubPid, Topic} -> SubOpts (src/emqx_broker.erl:80,
 * 101-102, 127-136, 150-158), non-shared subscriptions.  The defaults are
 * {qos 0, nl 0, rap 0, rh 0}, no subid (include/emqx_mqtt.hrl:207-211).
 * tm_subscribe_opts: emqx_broker:subscribe/3 (:127-136).  A new (topic,
 * subscriber) subscribes exactly as tm_subscribe does and stores opts; an
 * existing one merges as set_subopts/2 does (maps:merge(Old, New), :388-393):
 * qos, nl, rap and rh are replaced, subid only when non-zero
 * (with_subid(undefined, _), :139-142).  opts = NULL: the defaults.
 * tm_subscribe is tm_subscribe_opts with the defaults: on an existing
 * subscription it resets the four flags and keeps the subid.
 * tm_set_subopts: set_subopts/2 for a partial map -- only the fields named by
 * mask (TM_SUBOPT_*) change; TM_ENOENT when not subscribed (`false`).
 * tm_get_subopts: get_subopts/2 (:373-386); TM_ENOENT for `undefined`.
 * TM_EINVAL + tm_last_error(): qos > 2, nl > 1, rap > 1, rh > 2, a subid
 * above 268,435,455, an unknown mask bit, NULL opts where one is required
 * (tm_set_subopts), NULL out.  tm_unsubscribe and tm_subscriber_down delete the
 * options with the subscription.  All three work on a host-only engine. */
typedef struct {
    uint8_t  qos;    /* 0..2 */
    uint8_t  nl;     /* 0 | 1  No Local */
    uint8_t  rap;    /* 0 | 1  Retain As Published */
    uint8_t  rh;     /* 0..2   Retain Handling: stored and returned, not used on delivery */
    uint32_t subid;  /* 0 = none, else 1 .. 268,435,455 (the MQTT Subscription Identifier range) */
} tm_subopts;
#define TM_SUBOPT_QOS 1u
#define TM_SUBOPT_NL 2u
#define TM_SUBOPT_RAP 4u
#define TM_SUBOPT_RH 8u
#define TM_SUBOPT_SUBID 16u
#define TM_SUBID_MAX 268435455u
TM_API int tm_subscribe_opts(tm_engine* e, const uint8_t* topic, size_t len, uint32_t subscriber,
                             uint32_t node_dest, const tm_subopts* opts);
TM_API int tm_set_subopts(tm_engine* e, const uint8_t* topic, size_t len, uint32_t subscriber,
                          uint32_t mask, const tm_subopts* opts);
TM_API int tm_get_subopts(tm_engine* e, const uint8_t* topic, size_t len, uint32_t subscriber, tm_subopts* out);

/* Deliveries of a waited batch: dispatch(To, Delivery) (:284-309) for every
 * filter To matched by publish i (its local route, do_route/2 :243-244):
 * deliveries of row i = subscribers[row_offsets[i] .. row_offsets[i+1]), the
 * runs of its matched filters in match (Erlang binary) order, each run in
 * subscription order; row_offsets[i+1] - row_offsets[i] = DispN (0 =
 * {error, no_subscribers}).  match_offsets[j] (TM_DISPATCH_MATCH_OFFSETS) =
 * first delivery of match entry j, i.e. of filter ids[j] of tm_batch_result.
 * TM_DISPATCH_COUNT_ONLY: counts only, subscribers = NULL.
 * TM_DISPATCH_DEVICE: no copy back; the pointers are device memory of the
 * batch, valid until its next dispatch or re-prepare (match_offsets only with
 * TM_DISPATCH_MATCH_OFFSETS too: without it the engine skips making them
 * global).  Otherwise engine-owned
 * pinned memory valid likewise.  fill_ms = device time of the copy kernel.
 * TM_DISPATCH_ROWS (device only, implies TM_DISPATCH_DEVICE, excludes
 * MATCH_OFFSETS): the fan-out reads the walk's rows where it wrote them
 * (tm_batch_rows) instead of a dense CSR built first; the deliveries of row i
 * are then subscribers[row_offsets[i] .. row_offsets[i] + row_counts[i]) --
 * the same runs in the same order, rows no longer adjacent in publish order
 * (row_offsets has n_topics entries). */
typedef struct {
    uint32_t        n_topics;
    uint64_t        n_matches;
    uint64_t        n_deliveries;
    const uint64_t* row_offsets;    /* n_topics + 1 (TM_DISPATCH_ROWS: n_topics row starts) */
    const uint64_t* match_offsets;  /* n_matches + 1, or NULL */
    const uint32_t* subscribers;    /* n_deliveries, or NULL */
    float           fill_ms;
    const uint32_t* row_counts;     /* TM_DISPATCH_ROWS: deliveries of each row; otherwise NULL */
} tm_deliveries;
#define TM_DISPATCH_COUNT_ONLY    1u
#define TM_DISPATCH_MATCH_OFFSETS 2u
#define TM_DISPATCH_DEVICE        4u
#define TM_DISPATCH_ROWS          8u
TM_API int  tm_batch_dispatch(tm_engine* e, tm_batch* b, uint32_t flags, tm_deliveries* out);

/* Deliveries of a waited batch grouped by subscriber: what each SubPid's
 * mailbox holds after the batch's messages were published in order
 * (src/emqx_broker.erl:298-302) and what emqx_misc:drain_deliver/1 hands the
 * session as one list (src/emqx_misc.erl:128-142, src/emqx_connection.erl:376-378).
 * Let L be the batch's deliveries in tm_batch_dispatch order: publish order,
 * a publish's filters in match (Erlang binary) order, a filter's subscribers
 * in subscription order.  The inbox of subscriber S = subscribers[r] is
 * entries [inbox_offsets[r], inbox_offsets[r + 1]) of publishes / filter_ids:
 * the subsequence of L whose subscriber is S, in L's order.  A publish that
 * reaches S through two filters (a/+ and a/#) appears twice, in match order,
 * as the reference sends two messages.  This is SubPid's mailbox order when
 * one process publishes the batch's messages in order (Erlang keeps the
 * signal order between two processes); within one publish the reference
 * dispatches the filters in the order emqx_trie:match/1 found them (a DFS
 * over ETS lookups), which DESIGN.md §1 treats as a set -- here it is the
 * match order of tm_batch_result.
 * The call runs the fan-out itself (dense CSR, device-resident) and then a
 * stable radix sort by subscriber, so it counts as a dispatch of the batch:
 * pointers from an earlier tm_batch_dispatch or tm_batch_inboxes on the batch
 * are valid until the next of either, a re-prepare or a free.
 * TM_INBOX_DEVICE: no copy back, the four arrays are device memory of the
 * batch; otherwise batch-owned pinned memory, valid likewise.  passes = 8-bit
 * radix passes run: max(1, ceil(bits of the largest subscriber id ever given
 * to tm_subscribe, tm_shared_subscribe or their _opts forms / 8)); 0 when
 * there was nothing to sort.
 * n_topics = 0 or no delivery: n_subscribers = 0, inbox_offsets = {0}, rc 0.
 * TM_EINVAL + tm_last_error(): out NULL, an unknown flag, a batch not waited,
 * a TM_BATCH_DEDUP batch (an inbox entry names a publish, and a deduplicated
 * row is not one).  TM_ENODEV on a host-only engine.  TM_EOVERFLOW for more
 * than 2^32 - 16 deliveries (offsets and the sort's payload are u32). */
typedef struct {
    uint32_t        n_topics;       /* publishes of the batch */
    uint32_t        n_subscribers;  /* R: subscribers with at least one delivery */
    uint64_t        n_deliveries;   /* D: equals tm_batch_dispatch's n_deliveries */
    const uint32_t* subscribers;    /* R ids, strictly ascending */
    const uint32_t* inbox_offsets;  /* R + 1 */
    const uint32_t* publishes;      /* D: publish index of each delivery */
    const uint32_t* filter_ids;     /* D: the matched filter (To of {deliver, To, Msg}) */
    float           kernel_ms;      /* device time of the inbox kernels (not the fan-out before them) */
    uint32_t        passes;         /* radix passes run */
} tm_inboxes;
#define TM_INBOX_DEVICE 1u          /* no copy back: device pointers of the batch */
TM_API int tm_batch_inboxes(tm_engine* e, tm_batch* b, uint32_t flags, tm_inboxes* out);
/* diagnostic: deliveries per sort tile (tests place D around its multiples) */
TM_API uint32_t tm_inbox_tile(void);

/* What the session sends, per subscriber: the inboxes of tm_batch_inboxes on
 * the same batch (R subscribers, D deliveries, each inbox one drained
 * `Delivers` list in mailbox order) after the reference's two per-delivery
 * lookups of maps:find(To, Subscriptions), in the reference's order.
 * 1. emqx_channel:ignore_local/3 (src/emqx_channel.erl:682-693).  A delivery
 *    (publish i, filter To) of inbox S is *own* when the options of (S, To)
 *    have nl = 1 and from[i] == S; from[i] = TM_NONE is never own.  The
 *    reference uses lists:dropwhile: the LEADING RUN of own deliveries of the
 *    list is dropped and nothing after the first delivery that is not own --
 *    the default here.  TM_DELIVER_NL_ALL drops every own delivery
 *    (MQTT-3.8.3-3).  n_dropped_no_local counts the drops
 *    ('delivery.dropped.no_local').
 * 2. emqx_session:enrich_subopts/3 (src/emqx_session.erl:500-529) on every
 *    delivery left, with the options of (S, To): QoS = min(sub qos, publish
 *    qos), or max with TM_DELIVER_UPGRADE_QOS (#session.upgrade_qos, per call
 *    here); nl = 1 sets TM_MSG_NL whoever published (:510-511); the retain
 *    flag is the publish's when rap = 1, and also when rap = 0 and the publish
 *    has TM_MSG_RETAINED (:522-523), otherwise 0 (:524-525); subids[q] = the
 *    stored Subscription Identifier (TM_DELIVER_SUBIDS).
 * An inbox that loses every delivery disappears from subscribers /
 * inbox_offsets; the order inside an inbox is unchanged.  When nothing can
 * drop (no subscription has nl = 1, or from = NULL) subscribers,
 * inbox_offsets, publishes and filter_ids ARE the arrays of tm_batch_inboxes;
 * the options are still looked up for msg / subids (msg is uploaded, one
 * search per inbox and one per delivery run), so kernel_ms is not 0 on that
 * path, from = msg = NULL included.
 * The call runs tm_batch_inboxes itself, so it counts as a dispatch of the
 * batch: pointers of earlier dispatch / inboxes / deliver calls are valid
 * until the next of any of them, a re-prepare or a free.  Without
 * TM_DELIVER_DEVICE the results are batch-owned pinned memory.  Options
 * changed between two calls on the same waited batch are seen by the second.
 * TM_EINVAL + tm_last_error(): NULL out or opts, an unknown flag, a msg[i]
 * with QoS 3 or bits above 3, a batch not waited, a TM_BATCH_DEDUP batch.
 * TM_ENODEV on a host-only engine.  TM_EOVERFLOW as tm_batch_inboxes.  TM_EIO
 * + tm_last_error() if a (subscriber, filter) of the fan-out has no options
 * (both come from one host state under the engine lock). */
#define TM_MSG_RETAIN    4u  /* publish: #message.flags.retain; delivery: the flag after rap */
#define TM_MSG_RETAINED  8u  /* publish only: headers.retained =:= true */
#define TM_MSG_NL        8u  /* delivery only: emqx_message:set_flag(nl, Msg) */
#define TM_DELIVER_DEVICE      1u  /* no copy back: device pointers of the batch */
#define TM_DELIVER_UPGRADE_QOS 2u  /* #session.upgrade_qos = true */
#define TM_DELIVER_NL_ALL      4u  /* drop every own delivery, not only the leading run */
#define TM_DELIVER_SUBIDS      8u  /* fill subids[] */
typedef struct {
    const uint32_t* from;   /* n_topics host u32: the subscriber id of publish i's publisher; TM_NONE = none.
                               NULL = all TM_NONE */
    const uint8_t*  msg;    /* n_topics host bytes: bits 0-1 QoS, TM_MSG_RETAIN, TM_MSG_RETAINED; NULL = all 0 */
    uint32_t        flags;
} tm_deliver_opts;
typedef struct {
    uint32_t n_topics, n_subscribers;      /* R': subscribers with at least one delivery LEFT */
    uint64_t n_deliveries;                 /* D': deliveries left */
    uint64_t n_dropped_no_local;           /* D' + this = tm_batch_inboxes' D */
    const uint32_t* subscribers;           /* R', strictly ascending */
    const uint32_t* inbox_offsets;         /* R' + 1 */
    const uint32_t* publishes;             /* D' */
    const uint32_t* filter_ids;            /* D' */
    const uint8_t*  msg;                   /* D': bits 0-1 QoS, TM_MSG_RETAIN, TM_MSG_NL */
    const uint32_t* subids;                /* D' with TM_DELIVER_SUBIDS (0 = none), else NULL */
    float    kernel_ms;                    /* device time of the delivery kernels only (not the inboxes before them) */
} tm_session_inboxes;
TM_API int tm_batch_deliver(tm_engine* e, tm_batch* b, const tm_deliver_opts* opts, tm_session_inboxes* out);

/* The session's send window, per subscriber: what emqx_channel:handle_deliver/2
 * does with the list tm_batch_deliver leaves, one disposition per delivery.
 * The call runs tm_batch_deliver(dopts) itself; inboxes.* ARE that call's
 * arrays, nothing is reordered or compacted, and disp / packet_ids run
 * parallel to them (D').  TM_DELIVER_DEVICE in dopts is ignored: inboxes.* are
 * device pointers exactly when TM_WINDOW_DEVICE is set.  The session of inbox S is the entry of `sessions`
 * with that subscriber, or `defaults`: (P, F, L, M, flags) = (next_pkt_id,
 * inflight_free, mqueue_len, mqueue_max, flags).  qos = bits 0-1 of msg[q].
 * Connected channel (src/emqx_channel.erl:672-677): emqx_session:deliver/2
 * (src/emqx_session.erl:421-457).
 *   QoS 0 -> TM_DISP_SEND0, packet id 0 for `undefined` (:440-441).
 *   QoS 1/2, with a = the delivery's 0-based rank among the inbox's QoS > 0
 *   deliveries: a < F -> TM_DISP_SEND with id ((P - 1 + a) mod 65535) + 1
 *   (await/3 :535-537; next_pkt_id/1 :665-668 wraps 16#FFFF -> 1); otherwise
 *   the window is full (emqx_inflight:is_full/1, src/emqx_inflight.erl:83-87;
 *   it only fills during a batch, so it stays full) and the delivery enters
 *   the queue with queue rank j = a - F (:446-451).  F = TM_SESS_UNBOUNDED: a
 *   window of max size 0 is never full (src/emqx_inflight.erl:84-85).
 *   The new next_pkt_id is ((P - 1 + min(F, A)) mod 65535) + 1, A = the
 *   inbox's QoS > 0 deliveries.
 * Disconnected channel (TM_SESS_DISCONNECTED; src/emqx_channel.erl:659-663):
 * emqx_session:enqueue/2 (:459-472).  QoS 0 without TM_SESS_STORE_QOS0 ->
 * TM_DISP_DROP_QOS0 (emqx_mqueue:in/2's first clause, src/emqx_mqueue.erl:
 * 149-150); every other delivery enters the queue with its rank j among the
 * entering ones.  next_pkt_id is unchanged.
 * Queue (src/emqx_mqueue.erl:151-168, no priority table: PLen = len).  E
 * deliveries enter.  M > 0: drops = max(0, L + E - M) in 64 bits -- a full
 * queue drops its oldest for each message that enters (:160-165);
 * n_dropped_old = min(drops, L) come off the front of the queue the host
 * holds, and an entering delivery with j < drops - n_dropped_old was pushed
 * out by a later one: TM_DISP_DROP_FULL.  The others are TM_DISP_QUEUED.
 * M = 0 (?MAX_LEN_INFINITY): nothing drops.
 * TM_SESS_HOST: every delivery of the inbox is TM_DISP_HOST; the record keeps
 * P and holds zeros otherwise.
 * Not here: priority tables (tm_batch_window_prio, or TM_SESS_HOST), maybe_ack / maybe_nack of
 * shared deliveries (they enter the inboxes of an armed batch as plain
 * delivers, tm_batch_shared_mode).  Message expiry acts when the queue is
 * drained: tm_sessions_drain.
 * The call counts as a dispatch of the batch (pointer lifetime as
 * tm_batch_deliver).  The session table is uploaded per call: a second call
 * on the same waited batch with other sessions sees them.  Without
 * TM_WINDOW_DEVICE the results are batch-owned pinned memory.
 * Errors as tm_batch_deliver, and TM_EINVAL + tm_last_error() for sessions
 * not strictly ascending by subscriber, a next_pkt_id outside 1..65535
 * (defaults included), mqueue_len > mqueue_max with mqueue_max > 0, unknown
 * session or window flags, NULL sessions with n_sessions > 0, NULL wopts.
 * TM_ENODEV on a host-only engine.  TM_EIO + tm_last_error() if a kernel met
 * an index past D', R' or n_sessions. */
#define TM_SESS_DISCONNECTED 1u   /* conn_state = disconnected: the enqueue/2 path */
#define TM_SESS_STORE_QOS0   2u   /* #mqueue.store_qos0 */
#define TM_SESS_HOST         4u   /* leave this session to the host (it has a priority table) */
#define TM_SESS_UNBOUNDED    0xFFFFFFFFu  /* inflight_free when the window's max size is 0 */
#define TM_WINDOW_DEVICE     1u   /* no copy back: device pointers of the batch */
#define TM_DISP_SEND0     0u  /* QoS 0: sent with packet id `undefined` */
#define TM_DISP_SEND      1u  /* packet id assigned, inflight */
#define TM_DISP_QUEUED    2u  /* in the mqueue when the batch ends */
#define TM_DISP_DROP_QOS0 3u  /* 'delivery.dropped.qos0_msg' */
#define TM_DISP_DROP_FULL 4u  /* entered the queue, pushed out as the oldest: 'delivery.dropped.queue_full' */
#define TM_DISP_HOST      5u  /* TM_SESS_HOST */
#define TM_DISP_COUNT     6u
typedef struct {
    uint32_t subscriber;    /* the caller's id, as in tm_subscribe */
    uint32_t next_pkt_id;   /* 1..65535 */
    uint32_t flags;         /* TM_SESS_* */
    uint32_t inflight_free; /* max size - size of the inflight window, or TM_SESS_UNBOUNDED */
    uint32_t mqueue_len;    /* #mqueue.len now */
    uint32_t mqueue_max;    /* #mqueue.max_len; 0 = infinity */
} tm_session_state;
typedef struct {
    const tm_session_state* sessions;  /* n_sessions, strictly ascending by subscriber; NULL when 0 */
    uint32_t                n_sessions;
    tm_session_state        defaults;  /* for a subscriber not listed (subscriber field ignored) */
    uint32_t                flags;     /* TM_WINDOW_DEVICE */
} tm_window_opts;
typedef struct {
    uint32_t next_pkt_id;    /* the new value */
    uint32_t n_inflight;     /* deliveries that entered the window */
    uint32_t n_queued;       /* deliveries of this batch in the queue at the end */
    uint32_t n_dropped_old;  /* messages to pop from the front of the queue the host holds */
} tm_window_record;
typedef struct {
    tm_session_inboxes      inboxes;      /* tm_batch_deliver(dopts)'s result (device pointers with TM_WINDOW_DEVICE) */
    const uint8_t*          disp;         /* D': TM_DISP_* */
    const uint16_t*         packet_ids;   /* D': 0 unless disp is TM_DISP_SEND */
    const tm_window_record* records;      /* R' */
    uint64_t                totals[TM_DISP_COUNT];   /* deliveries per disposition */
    float                   kernel_ms;    /* device time of the window kernels only */
    uint32_t                pad0;
} tm_session_window;
TM_API int tm_batch_window(tm_engine* e, tm_batch* b, const tm_deliver_opts* dopts, const tm_window_opts* wopts,
                           tm_session_window* out);

/* The send window of sessions whose mqueue has a priority table
 * (#mqueue.p_table, src/emqx_mqueue.erl:151-168, 195-196; the zone settings
 * mqueue_priorities / mqueue_default_priority, src/emqx_session.erl:179-180).
 * A table (tm_ptable) maps topics to priorities 0..255 or TM_PRIO_INFINITY;
 * Priority = get_priority(Topic, PTab, Dp) compares the publish's topic BYTES
 * with the keys (maps:get/3, no wildcard) and gives default_priority (0 for
 * `lowest`, TM_PRIO_INFINITY for `highest`, or an integer) to a topic the
 * table lacks -- an empty table included (:196).  A session without a table
 * (?NO_PRIORITY_TABLE) always uses priority 0 (:195) and is what
 * tm_batch_window computes.
 * tm_ptable_create: n keys, key i = topics[offsets[i] .. offsets[i + 1]); a
 * repeated key keeps its last priority (maps:put).  The table's CLASSES are
 * its distinct priorities together with its default, descending, infinity
 * first: class 0 is the highest.  tm_ptable_classes writes them (as given:
 * 0..255 or TM_PRIO_INFINITY) and returns their number.  The table belongs to
 * the engine it was made for and is freed with tm_ptable_free before that
 * engine is closed, as a tm_acl; both calls work on a host-only engine.  The
 * host builds the open-addressed image the lookup kernel probes here, once.
 * TM_EINVAL + tm_last_error(): a priority above 255 that is not
 * TM_PRIO_INFINITY (the default included), more than TM_PRIO_MAX_CLASSES
 * classes, a key over TM_MAX_TOPIC_LEN bytes, offsets not monotone.
 * The two caps are design limits, not measurements: eight classes keep the
 * per-inbox class record at 64 B and the per-round work at one ballot per
 * class (the reference's own tables hold three priorities); sixteen tables
 * bound the per-publish class bytes of one call.
 *
 * tm_batch_window_prio is tm_batch_window with tables.  The table of inbox S
 * is tables[prio entry of S .table] when `prio` lists S, else
 * tables[default_table] (TM_NONE: no table); a prio entry may name TM_NONE
 * itself (that session has no table, its plen is ignored).  TM_SESS_HOST wins
 * over a table.  Every priority class of a session is a bounded queue of its
 * own: max_len bounds each priority separately (PLen =:= MaxLen with PLen =
 * emqx_pqueue:plen(Priority, Q), :159-165), the message pushed out is the
 * oldest of that priority (emqx_pqueue:out/2), and len is the sum.  Which
 * deliveries are TM_DISP_SEND0 / SEND / DROP_QOS0 is decided exactly as in
 * tm_batch_window, whatever the priority (the QoS-0 clause :149-150 comes
 * first).  Of the entering deliveries class c has E_c; with L_c = plen[c]
 * (0 for a session not in `prio`) and M = mqueue_max, in 64 bits:
 *   drops_c = max(0, L_c + E_c - M) when M > 0, else 0
 *   n_dropped_old_c = min(drops_c, L_c);  dnew_c = drops_c - n_dropped_old_c
 * and an entering delivery whose 0-based rank among the entering deliveries
 * of its inbox and class is below dnew_c is TM_DISP_DROP_FULL, the others
 * TM_DISP_QUEUED.  out is filled exactly as tm_batch_window fills it; a tabled
 * session's record holds the sums over its classes.  pout->pclass[q] is the
 * class of delivery q in its session's table, for every delivery of a tabled
 * session, sent or not; TM_PRIO_NOCLASS for a session without a table or with
 * TM_SESS_HOST.  pout->precords[r * TM_PRIO_MAX_CLASSES + c] are class c's
 * {n_queued, n_dropped_old} of inbox r: zeros for classes the table lacks and
 * for sessions without a table.  A session without a table gets bit for bit
 * what tm_batch_window gives it (n_tables = 0: every session).
 * The classes come from a lookup kernel over the batch's device-resident topic
 * bytes (lookup_kernel_ms; out->kernel_ms is the window kernels' time), so a
 * batch made by tm_batch_prepare_tokens, which has none, is refused.  An
 * armed batch (tm_batch_shared_mode) needs nothing extra: a shared delivery's
 * topic is its publish's.  Memory mode and pointer lifetime follow
 * TM_WINDOW_DEVICE in wopts, as for tm_batch_window; pclass and precords are
 * device pointers exactly when the other results are.
 * Errors as tm_batch_window (mqueue_len > mqueue_max is legal for a tabled
 * session: each class is bounded, not the sum), and TM_EINVAL +
 * tm_last_error() for NULL popts or pout, n_tables > TM_PRIO_MAX_TABLES, a
 * NULL table or one of another engine, a table index >= n_tables that is not
 * TM_NONE, prio not strictly ascending by subscriber, a prio subscriber
 * missing from wopts->sessions, sum of plen != mqueue_len, plen[c] >
 * mqueue_max when mqueue_max > 0, plen[c] != 0 for a class the table lacks, a
 * tabled session (or tabled defaults) with mqueue_len > 0 and no prio entry
 * (TM_SESS_HOST sessions are exempt from these four), a batch without a
 * device copy of its topic bytes.  TM_ENODEV on a host-only engine.
 * Not here: more than TM_PRIO_MAX_CLASSES classes, the group / sharded /
 * multi-process forms, maybe_ack / maybe_nack.  Message expiry acts when the
 * queue is drained: tm_sessions_drain. */
#define TM_PRIO_INFINITY    0xFFFFu  /* the priority `infinity` */
#define TM_PRIO_MAX_CLASSES 8u       /* classes of one table (distinct priorities + default) */
#define TM_PRIO_MAX_TABLES  16u      /* tables of one tm_batch_window_prio call */
#define TM_PRIO_NOCLASS     0xFFu    /* pclass of a delivery whose session has no table */
typedef struct tm_ptable tm_ptable;
TM_API int tm_ptable_create(tm_engine* e, const uint8_t* topics, const uint64_t* offsets, const uint16_t* priorities,
                            uint32_t n, uint32_t default_priority, tm_ptable** table);
TM_API void tm_ptable_free(tm_engine* e, tm_ptable* table);
TM_API uint32_t tm_ptable_classes(const tm_ptable* table, uint16_t out[TM_PRIO_MAX_CLASSES]);
typedef struct {
    uint32_t subscriber;                  /* the caller's id, as in tm_session_state */
    uint32_t table;                       /* index into tables[], or TM_NONE: no table */
    uint32_t plen[TM_PRIO_MAX_CLASSES];   /* messages of class c in the queue now; their sum is mqueue_len */
} tm_session_prio;
typedef struct {
    tm_ptable* const*      tables;        /* n_tables; NULL when 0 */
    uint32_t               n_tables;
    uint32_t               n_prio;
    const tm_session_prio* prio;          /* n_prio, strictly ascending by subscriber; NULL when 0 */
    uint32_t               default_table; /* index into tables[] or TM_NONE: subscribers not listed in prio */
    uint32_t               pad0;          /* 0 */
} tm_window_prio_opts;
typedef struct {
    uint32_t n_queued;       /* deliveries of this batch and class in the queue at the end */
    uint32_t n_dropped_old;  /* messages to pop from the front of that class's queue */
} tm_prio_record;
typedef struct {
    const uint8_t*        pclass;           /* D' */
    const tm_prio_record* precords;         /* R' x TM_PRIO_MAX_CLASSES */
    float                 lookup_kernel_ms; /* device time of the class lookup */
    uint32_t              pad0;
} tm_window_prio;
TM_API int tm_batch_window_prio(tm_engine* e, tm_batch* b, const tm_deliver_opts* dopts, const tm_window_opts* wopts,
                                const tm_window_prio_opts* popts, tm_session_window* out, tm_window_prio* pout);

/* ---- session drain: dequeue after acks, message expiry ----------------- */
/* What emqx_session:puback/2 and pubcomp/2 do once an inflight slot is free:
 * dequeue/1 (src/emqx_session.erl:389-413) over the mqueue the host holds, for
 * a batch of sessions, one disposition per queued message.  Stand-alone as
 * tm_acl_check: caller-owned host arrays in and out, synchronous, serialised
 * on the engine's mutex; it runs on the engine's first replica.
 * in: session r is {next_pkt_id P, inflight_free F} (F = max size - size of
 * the inflight window once the host took the acked ids out, batch_n/1 :680-684)
 * and owns messages q_off[r] .. q_off[r + 1] of the message arrays, listed in
 * ARRIVAL order -- the order emqx_mqueue:in/2 saw them, which is the order
 * tm_batch_window_prio reported them TM_DISP_QUEUED with their pclass.  The
 * priority order is worked out here, not by the host.  qmsg[m]: bits 0-1 the
 * QoS, TM_QMSG_EXPIRY when the message's properties hold
 * 'Message-Expiry-Interval', bits 4-6 its class (0 the highest, as
 * tm_ptable_classes orders them; 0 for a session without a table); the other
 * bits are 0.  created_ms[m] is #message.timestamp, expiry_s[m] the interval,
 * now_ms erlang:system_time(millisecond) taken once for the call.
 * Expiry (src/emqx_message.erl:224-228, 296-297): elapsed = max(0, now_ms -
 * created_ms); a message with TM_QMSG_EXPIRY is expired iff elapsed >
 * expiry_s * 1000, in 64 bits.  Without the flag it never is, whatever the two
 * arrays hold for it.
 * Out order (emqx_mqueue:out/1, src/emqx_mqueue.erl:170-176, over
 * emqx_pqueue:out/1): the session's messages stably sorted by class.
 * dequeue(Cnt, ...) with Cnt = F, or TM_DRAIN_BATCH_N for TM_SESS_UNBOUNDED
 * (?DEFAULT_BATCH_N, :153): it pops in out order, throws expired messages
 * away (:404-406), counts down on every other message of QoS > 0 (acc_cnt/2
 * :411-413) and stops at 0 (:397-398) or at the end of the queue (:402).  A
 * message is COUNTED when it is not expired and its QoS is above 0.  With
 * C(m) = the session's counted messages in classes above m's plus those of
 * m's class before m in arrival order, and U(m) the same over the messages
 * not expired: m is popped iff C(m) < Cnt.  A QoS 0 or expired message behind
 * the Cnt-th counted one stays (dequeue(0, ...) stops at once).
 *   popped and expired -> TM_DRAIN_EXPIRED ('delivery.dropped.expired')
 *   popped, QoS 0      -> TM_DRAIN_SEND0, packet id 0 (deliver_msg/2 :440-441)
 *   popped, counted    -> TM_DRAIN_SEND, packet id ((P - 1 + C(m) mod 65535)
 *                         mod 65535) + 1 (:453-456, next_pkt_id/1 :665-669);
 *                         the window has Cnt free slots, so nothing is queued
 *                         again
 *   not popped         -> TM_DRAIN_KEPT
 * order[m] = U(m) for a TM_DRAIN_SEND / TM_DRAIN_SEND0 message, its place in
 * the session's publish list (deliver/3 :429-438); TM_DRAIN_NO_ORDER
 * otherwise.  expiry_out[m] (the array may be NULL) is what
 * emqx_message:update_expiry/1 leaves in a sent message that has the flag
 * (src/emqx_channel.erl:814, src/emqx_message.erl:230-239): max(1, expiry_s -
 * elapsed div 1000) when elapsed > 0, else expiry_s; for every other message
 * the input value (0 when expiry_s is NULL).
 * records[r] = {the new next_pkt_id ((P - 1 + n_send mod 65535) mod 65535) + 1,
 * n_send, n_send0, n_expired}; popped[r * TM_PRIO_MAX_CLASSES + c] = how many
 * messages to take off the front of class c of the queue the host holds,
 * their sum n_send + n_send0 + n_expired.  Cnt = 0 or an empty queue
 * (is_empty/1 :390-391): nothing is popped, next_pkt_id stays.  totals[] are
 * the messages per disposition; kernel_ms the device time (HIP events) of the
 * drain kernels only.
 * TM_EINVAL + tm_last_error(): NULL in or out; n_sessions > 0 with NULL
 * sessions, q_off, records or popped; Q = q_off[n_sessions] > 0 with NULL
 * qmsg, disp, packet_ids or order; a next_pkt_id outside 1..65535; offsets not
 * monotone or not starting at 0; Q >= 2^32; QoS 3; a reserved bit of qmsg or
 * pad0 set; a message with
 * TM_QMSG_EXPIRY while created_ms or expiry_s is NULL.  All of them are found
 * before anything runs, on a host-only engine too; then TM_ENODEV on a
 * host-only engine.  TM_EIO + tm_last_error() if a kernel met an index past Q
 * or n_sessions.  n_sessions = 0 is TM_OK with zero totals.
 * Not here: retry/1 over the inflight window, maybe_ack / maybe_nack, more
 * than TM_PRIO_MAX_CLASSES classes, device-pointer outputs, the group /
 * sharded forms, a split over replicas. */
#define TM_QMSG_EXPIRY     4u           /* qmsg: the message has a Message-Expiry-Interval */
#define TM_QMSG_CLASS_SHIFT 4u          /* qmsg: bits 4-6 the class */
#define TM_DRAIN_BATCH_N   1000u        /* ?DEFAULT_BATCH_N: Cnt of a window of max size 0 */
#define TM_DRAIN_NO_ORDER  0xFFFFFFFFu  /* order[] of a message that is not sent */
#define TM_DRAIN_SEND0     0u  /* QoS 0: sent with packet id `undefined` */
#define TM_DRAIN_SEND      1u  /* packet id assigned, inflight */
#define TM_DRAIN_KEPT      2u  /* still in the mqueue */
#define TM_DRAIN_EXPIRED   3u  /* popped and thrown away: 'delivery.dropped.expired' */
#define TM_DRAIN_COUNT     4u
typedef struct {
    uint32_t next_pkt_id;   /* 1..65535 */
    uint32_t inflight_free; /* max size - size of the inflight window, or TM_SESS_UNBOUNDED */
} tm_drain_session;
typedef struct {
    const tm_drain_session* sessions;   /* n_sessions */
    const uint64_t*         q_off;      /* n_sessions + 1, monotone from 0; q_off[n_sessions] = Q < 2^32 */
    const uint8_t*          qmsg;       /* Q */
    const int64_t*          created_ms; /* Q; may be NULL when no message has TM_QMSG_EXPIRY */
    const uint32_t*         expiry_s;   /* Q; may be NULL when no message has TM_QMSG_EXPIRY */
    int64_t                 now_ms;
    uint32_t                n_sessions;
    uint32_t                pad0;       /* 0 */
} tm_drain_in;
typedef struct {
    uint32_t next_pkt_id;   /* the new value */
    uint32_t n_send;        /* TM_DRAIN_SEND messages: they enter the inflight window */
    uint32_t n_send0;       /* TM_DRAIN_SEND0 messages */
    uint32_t n_expired;     /* TM_DRAIN_EXPIRED messages */
} tm_drain_record;
typedef struct {
    uint8_t*         disp;        /* Q: TM_DRAIN_* */
    uint16_t*        packet_ids;  /* Q: 0 unless disp is TM_DRAIN_SEND */
    uint32_t*        order;       /* Q */
    uint32_t*        expiry_out;  /* Q, or NULL: not wanted */
    tm_drain_record* records;     /* n_sessions */
    uint32_t*        popped;      /* n_sessions x TM_PRIO_MAX_CLASSES */
    uint64_t         totals[TM_DRAIN_COUNT];   /* messages per disposition */
    float            kernel_ms;   /* device time of the drain kernels only */
    uint32_t         pad0;
} tm_drain_out;
TM_API int tm_sessions_drain(tm_engine* e, const tm_drain_in* in, tm_drain_out* out);

/* ---- shared subscriptions: emqx_shared_sub dispatch on the device ------ */
/* The ?SHARED_SUBS bag ({Group, Topic} -> SubPid, src/emqx_shared_sub.erl:
 * 287-305) of the local node.  group_dest = the aggregated dest id the caller
 * uses for {Group, _} in tm_route_add (emqx_broker:aggre/1), so the ids in
 * tm_routes.dests and the group ids here are the same; subscriber ids are the
 * caller's.  All four calls work on a host-only engine.
 * tm_shared_subscribe: handle_call({subscribe, Group, Topic, SubPid})
 * (:297-305): the first member of (group, topic) adds the route (topic,
 * group_dest) (:299-302); a repeated (group, topic, subscriber) is a no-op (a
 * bag stores an object once, :304); members keep insertion order. */
TM_API int  tm_shared_subscribe(tm_engine* e, const uint8_t* topic, size_t len, uint32_t group_dest,
                                uint32_t subscriber);
/* handle_call({unsubscribe, Group, Topic, SubPid}) (:307-315): TM_ENOENT if
 * the subscriber is not a member (delete_object of no record); the last
 * member deletes the route (:310-313). */
TM_API int  tm_shared_unsubscribe(tm_engine* e, const uint8_t* topic, size_t len, uint32_t group_dest,
                                  uint32_t subscriber);
/* cleanup_down/1 (:358-367): drops every shared membership of the subscriber;
 * *n_removed (may be NULL) = how many.  The non-shared bag is not touched
 * (that is tm_subscriber_down). */
TM_API int  tm_shared_member_down(tm_engine* e, uint32_t subscriber, uint64_t* n_removed);
/* subscribers/2 (:277-278): the members of (group, topic) in insertion order;
 * writes up to cap ids, *n = full count (0 for an unknown group or topic). */
TM_API int  tm_shared_members(tm_engine* e, const uint8_t* topic, size_t len, uint32_t group_dest,
                              uint32_t* buf, uint32_t cap, uint32_t* n);
/* emqx_broker:subscribe/3 with share => Group (src/emqx_broker.erl:127-136,
 * 145-163): ?SUBOPTION has one entry per {SubPid, Topic}, shared or not, Topic
 * being the filter without its $share/Group/ prefix, so the options are stored
 * under (subscriber, topic) -- the table tm_batch_deliver searches -- marked
 * as owned by the membership in group_dest (the `share` key); then the call
 * does what tm_shared_subscribe does.  opts = NULL: the defaults.
 * If (subscriber, topic) already has options, stored by tm_subscribe(_opts) or
 * by an earlier shared subscribe of any group, the reference takes its
 * `true -> %% Existed` branch (:129-135): ONLY the options merge, as
 * tm_subscribe_opts merges them, and no membership changes -- the subscriber
 * does not join group_dest.  Likewise tm_subscribe(_opts) on a (subscriber,
 * topic) whose options a shared subscribe stored only merges.
 * tm_shared_unsubscribe and tm_shared_member_down delete the options that a
 * shared subscribe of that group stored (do_unsubscribe/3, :179-183), never
 * those of a non-shared subscription; tm_get_subopts / tm_set_subopts work on
 * such an entry unchanged.  tm_shared_subscribe stores no options: a member
 * without an entry is legal (see tm_batch_shared_mode).  TM_EINVAL as
 * tm_subscribe_opts.  Works on a host-only engine. */
TM_API int  tm_shared_subscribe_opts(tm_engine* e, const uint8_t* topic, size_t len, uint32_t group_dest,
                                     uint32_t subscriber, const tm_subopts* opts);

/* dispatch(Group, To, Delivery) (:110-125) for every {To, Group} route of every
 * publish of a waited batch (do_route/2, src/emqx_broker.erl:245-248): one
 * delivery (filter id, group id, subscriber) per (publish, matched filter,
 * group on that filter), the subscriber picked by pick_subscriber/5
 * (:260-275): lists:nth(Nth, Members) over the group's Count members, a
 * one-member group always that member without touching any state (:260).
 * Row i = deliveries [row_offsets[i], row_offsets[i+1]): filters in match
 * (Erlang binary) order, a filter's groups in first-added order -- the order of
 * tm_routes.
 *   TM_SHARED_HASH (:267-268): Nth = 1 + keys[i] rem Count; the caller passes
 *     erlang:phash2(ClientId) of publish i, which makes the pick the
 *     reference's, bit for bit.
 *   TM_SHARED_ROUND_ROBIN (:269-275): one 64-bit cursor per (group, topic), per
 *     replica, in HBM; a pick takes the next cursor value c and Nth = 1 + c
 *     rem Count; the first pick ever is member 1.  When Count changed since
 *     the last pick the next pick is (previous pick index + 1) rem NewCount,
 *     the reference's (N + 1) rem Count on the stored remainder.  Which
 *     publish of a batch gets which cursor value is unordered; the multiset of
 *     a batch's picks is exactly the next K cursor values.  (The reference
 *     keeps the counter in each publishing process's dictionary; a batch has
 *     no publisher identity.)
 *   TM_SHARED_RANDOM (:265-266): rand:uniform/1 has no reproducible answer;
 *     here Nth = 1 + (r >> 32) rem Count with, in wrapping u64 arithmetic,
 *       G = 0x9E3779B97F4A7C15
 *       mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *               z *= 0x94D049BB133111EB; z ^= z >> 31
 *       r = mix((mix(seed + G * (i + 1)) ^ (filter id << 32 | group id)) + G)
 *     for publish index i: reproducible for a seed, uniform over the members.
 * TM_SHARED_COUNT_ONLY: row_offsets and n_deliveries only, no pick (a
 * round-robin cursor does not move), the three arrays NULL.
 * TM_SHARED_DEVICE: no copy back; the pointers are device memory of the batch.
 * Otherwise batch-owned pinned memory.  Both valid until the batch's next
 * tm_batch_dispatch_shared, re-prepare or free.  kernel_ms = device time of
 * the count, scan and pick kernels.
 * TM_EINVAL + tm_last_error(): batch not waited, unknown strategy or flag,
 * TM_SHARED_HASH without keys, a TM_BATCH_DEDUP batch (the pick is per
 * publish).  TM_ENODEV on a host-only engine.  TM_EOVERFLOW for more than
 * 2^32 - 16 deliveries. */
#define TM_SHARED_RANDOM      0u
#define TM_SHARED_ROUND_ROBIN 1u
#define TM_SHARED_HASH        2u
#define TM_SHARED_COUNT_ONLY  1u
#define TM_SHARED_DEVICE      2u
typedef struct {
    uint32_t        strategy;   /* TM_SHARED_RANDOM | _ROUND_ROBIN | _HASH */
    uint32_t        flags;      /* TM_SHARED_COUNT_ONLY | TM_SHARED_DEVICE */
    const uint32_t* keys;       /* TM_SHARED_HASH: n_topics host keys, one per publish */
    uint64_t        seed;       /* TM_SHARED_RANDOM */
} tm_shared_opts;
typedef struct {
    uint32_t        n_topics;
    uint64_t        n_deliveries;
    const uint32_t* row_offsets;  /* n_topics + 1 */
    const uint32_t* filter_ids;   /* n_deliveries, or NULL */
    const uint32_t* groups;       /* n_deliveries, or NULL */
    const uint32_t* subscribers;  /* n_deliveries, or NULL */
    float           kernel_ms;
} tm_shared_deliveries;
TM_API int  tm_batch_dispatch_shared(tm_engine* e, tm_batch* b, const tm_shared_opts* opts,
                                     tm_shared_deliveries* out);

/* Shared deliveries in the inboxes.  emqx_shared_sub:do_dispatch/4
 * (src/emqx_shared_sub.erl:135-158, shared_dispatch_ack_enabled = false) ends
 * in the same SubPid ! {deliver, Topic, Msg} as emqx_broker:dispatch/3, so a
 * member's mailbox holds both kinds in one list, and ignore_local/3,
 * enrich_subopts/3, next_pkt_id and the inflight window run over that list.
 * tm_batch_shared_mode arms a prepared batch (opts = NULL disarms it; an
 * unarmed batch behaves bit for bit as before).  While armed,
 * tm_batch_inboxes, tm_batch_deliver and tm_batch_window on the batch work on
 * the merged list L' instead of L: publishes in order; within a publish its
 * match entries in match order; within a match entry first the subscribers of
 * tm_batch_dispatch in subscription order (the {To, node()} route:
 * lists:usort orders an atom before a tuple, src/emqx_broker.erl:255-261),
 * then one picked member per group of tm_batch_dispatch_shared, in its order.
 * The inbox of S is the subsequence of L' addressed to S.  n_deliveries is
 * D + D_shared; TM_EOVERFLOW above 2^32 - 16 for the sum.  With no group
 * anywhere L' is L.
 * opts: strategy and seed as tm_batch_dispatch_shared; keys (TM_SHARED_HASH,
 * n_topics host words) are COPIED at the call, so arm again after a
 * re-prepare with another publish count (the calls return TM_EINVAL until
 * then).  Each of the three calls runs the pick itself, as it runs the
 * fan-out itself: with TM_SHARED_ROUND_ROBIN every call takes fresh cursor
 * values, exactly as every tm_batch_dispatch_shared does (deliver + window on
 * one batch are two picks; tm_batch_window alone is one), and which publish
 * gets which cursor value is unordered.  An armed call also counts as a
 * tm_batch_dispatch_shared of the batch for that call's pointer lifetime.
 * Options: a shared delivery (S, To) looks up (S, To) in the table
 * tm_batch_deliver searches.  A member without an entry is legal: its
 * delivery passes through unenriched (get_subopts/2 = [], enrich_subopts([],
 * Msg, _) leaves the message alone, src/emqx_session.erl:500-509) -- the
 * publish's QoS and retain flag, no TM_MSG_NL, subid 0, never own.  A
 * non-shared delivery without options stays TM_EIO.  A shared delivery with
 * nl = 1 from its own publisher is own.  TM_EIO + tm_last_error() if a pick
 * found a group without a member.
 * TM_EINVAL + tm_last_error(): unknown strategy or flag, TM_SHARED_COUNT_ONLY
 * or TM_SHARED_DEVICE (no meaning here), TM_SHARED_HASH without keys, a
 * TM_BATCH_DEDUP batch.  TM_ENODEV on a host-only engine.
 * Not here: dispatch_with_ack/3 (shared_dispatch_ack_enabled = true), sticky. */
TM_API int  tm_batch_shared_mode(tm_engine* e, tm_batch* b, const tm_shared_opts* opts);
/* groups[q] = the group id of delivery q of the batch's most recent
 * tm_batch_inboxes / tm_batch_deliver / tm_batch_window call, TM_NONE for an
 * ordinary delivery: parallel to that call's publishes / filter_ids, compacted
 * with them after deliver's No Local drops.  TM_INBOX_DEVICE: a device
 * pointer; otherwise batch-owned pinned memory; both valid as that call's
 * arrays.  TM_EINVAL on an unarmed batch, or when no such call ran armed. */
TM_API int  tm_batch_inbox_groups(tm_engine* e, tm_batch* b, uint32_t flags, const uint32_t** groups);

/* ---- bulk load + filter-sharded mode ------------------ */
/* emqx_trie:insert/1 over n filters (filters = concatenated bytes, offsets[n+1]).
 * nshards <= 1: every filter.  Otherwise only the filters whose
 * tm_filter_shard() is `shard` or nshards (replicated); *n_inserted (may be
 * NULL) counts them.  Stops at the first error.  A batch of >= 2,048
 * filters on a big trie is applied by parallel workers: after an error the
 * filters applied are each worker's finished ones (every filter is applied
 * whole or not at all, the trie stays consistent), so a subset of the batch
 * that need not be a prefix; *n_inserted counts them and re-applying the
 * batch is idempotent (emqx_trie:insert/1 is). */
TM_API int  tm_trie_insert_many(tm_engine* e, const uint8_t* filters, const uint64_t* offsets,
                                uint32_t n, uint32_t shard, uint32_t nshards, uint64_t* n_inserted);
/* emqx_trie:delete/1 over n filters; *n_deleted (may be NULL) counts the calls
 * made.  Stops at the first error (subset semantics of a parallel batch as
 * for tm_trie_insert_many). */
TM_API int  tm_trie_delete_many(tm_engine* e, const uint8_t* filters, const uint64_t* offsets, uint32_t n,
                                uint64_t* n_deleted);
/* One subscription delta: tm_trie_delete_many(del...) then
 * tm_trie_insert_many(ins..., 0, 1), with the two lists planned together (one
 * pass of the workers over both; an insert whose planned node a delete of the
 * same call removed walks again).  The result equals the two calls in that
 * order, filter for filter: emqx_trie:delete/1 then insert/1
 * (src/emqx_trie.erl:81-116) as a session's unsubscribe + subscribe batch
 * reaches the router (src/emqx_router.erl:113-124, 163-169).  A delete error
 * returns before any insert; *n_deleted / *n_inserted (may be NULL) count as
 * the two calls do. */
TM_API int  tm_trie_apply_many(tm_engine* e, const uint8_t* del_filters, const uint64_t* del_offsets, uint32_t n_del,
                               const uint8_t* ins_filters, const uint64_t* ins_offsets, uint32_t n_ins,
                               uint64_t* n_deleted, uint64_t* n_inserted);
/* Interns n words in order (the shared dictionary of the sharded mode).  Words
 * must not contain '/'; '', "+" and "#" have fixed ids and are skipped. */
TM_API int  tm_dict_load(tm_engine* e, const uint8_t* words, const uint64_t* offsets, uint32_t n);
/* Shard of a filter among nshards: filters of >= 2 levels whose first two
 * levels are literal words live on shard hash(id(w0), id(w1)) mod nshards; all
 * others return nshards (replicated on every shard).  A publish whose first two
 * words are known literals can only be matched by filters of its own shard or
 * replicated ones, so one shard resolves it completely. */
TM_API int  tm_filter_shard(tm_engine* e, const uint8_t* filter, size_t len, uint32_t nshards);
/* Host tokenisation (emqx_topic:words/1 + interning): words[] = (class << 29 |
 * word id) per level, toff[n+1] word offsets, tflags[n] (bit 0: '$' topic, bit
 * 1: generic path).  *nwords_out = total words; TM_EOVERFLOW if > words_cap. */
TM_API int  tm_tokenize(tm_engine* e, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                        uint32_t* words, uint64_t words_cap, uint32_t* toff, uint8_t* tflags,
                        uint64_t* nwords_out);
/* tm_tokenize on the device (the tokeniser tm_match_batch uses by default):
 * the host topic bytes are copied to HBM and tokenised against the device
 * mirror of the word dictionary into caller DEVICE buffers words[words_cap],
 * toff[n+1], tflags[n] -- the same values tm_tokenize writes.  *nwords_out =
 * total words; TM_EOVERFLOW (nothing past words_cap written) if > words_cap.
 * Returns when done.  Replaces emqx_topic:words/1 (src/emqx_topic.erl:150-164)
 * for a whole batch. */
TM_API int  tm_tokenize_device(tm_engine* e, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                               uint32_t* d_words, uint64_t words_cap, uint32_t* d_toff, uint8_t* d_tflags,
                               uint64_t* nwords_out);
/* A batch from tokenised arrays (tm_tokenize layout).  on_device = 1: the
 * pointers are device memory of this engine's GPU (e.g. received from another
 * shard); they are copied (and validated on the device: TM_EINVAL for offsets
 * that are not monotone from 0 to nwords or unflagged deep topics), so the
 * caller may reuse them once this returns.  A non-NULL *out is re-prepared in
 * place (its buffers only grow); NULL allocates a new batch. */
TM_API int  tm_batch_prepare_tokens(tm_engine* e, const uint32_t* words, const uint32_t* toff,
                                    const uint8_t* tflags, uint32_t n, uint64_t nwords, int on_device,
                                    tm_batch** out);
/* Device kernel: shard[t] = the shard owning tokenised topic t (tm_filter_shard's
 * rule applied to its first two words), or nshards when any shard resolves it
 * (only replicated filters can match).  Device pointers; returns when done. */
TM_API int  tm_tokens_shard(tm_engine* e, const uint32_t* d_words, const uint32_t* d_toff, uint32_t n,
                            uint32_t nshards, uint32_t* d_shard);
/* Writes the batch's per-topic match counts and its filter ids mapped to
 * id * mul + add (global ids of a shard) into caller device buffers
 * (counts[n], ids[n_matches]) on the engine stream; returns when done. */
TM_API int  tm_batch_export(tm_engine* e, tm_batch* b, uint32_t* d_counts, uint32_t* d_ids,
                            uint32_t mul, uint32_t add);

/* Device row gather (the exchange's reorder step): for i < n, copies the u32
 * row src[src_off[idx[i]] .. src_off[idx[i] + 1]) to dst[dst_off[i] ..).  All
 * pointers are device memory; offsets and indices are int64.  Returns when done. */
TM_API int  tm_gather_rows(tm_engine* e, const uint32_t* d_src, const int64_t* d_src_off, const int64_t* d_idx,
                           uint32_t n, const int64_t* d_dst_off, uint32_t* d_dst);

/* ---- filters ---------------------------------------------------------- */
/* Bytes of a filter id returned by a match (the #trie_node.topic binary).
 * A matched id keeps naming its filter while the result that holds it is
 * valid, even if the filter is deleted meanwhile: ids freed by deletes are
 * reused only after every batch launched before the delete has been
 * re-launched or freed.  The pointer is into engine memory that a later
 * insert may move: callers racing with writers use tm_filter_copy. */
TM_API const uint8_t* tm_filter_bytes(tm_engine* e, uint32_t id, size_t* len);
/* Copies the bytes of filter `id` into buf[cap] under the engine lock; *len =
 * its length (copied only if <= cap).  TM_ENOENT if the id never named a
 * filter or was reused for a node without one. */
TM_API int  tm_filter_copy(tm_engine* e, uint32_t id, uint8_t* buf, size_t cap, size_t* len);
/* Bulk tm_filter_copy under one acquisition of the engine lock (a result row
 * turned into filter binaries).  *need = the bytes of every id still naming a
 * filter; if *need > cap nothing is copied (grow buf and call again).
 * Otherwise the live filters are packed into buf in id order: filter k is
 * buf[offs[k], offs[k+1]), *n_out = count (offs holds n+1 entries); ids no
 * longer naming a filter are skipped, and keep[k] (may be NULL) = the index
 * in ids of filter k. */
TM_API int  tm_filters_copy(tm_engine* e, const uint32_t* ids, uint32_t n, uint8_t* buf, size_t cap,
                            uint64_t* offs, uint32_t* keep, uint32_t* n_out, uint64_t* need);
/* tm_filters_copy over ids packed id_bytes (3 or 4) bytes each, as
 * tm_match_batch_packed returns them (no unpack pass). */
TM_API int  tm_filters_copy_packed(tm_engine* e, const uint8_t* ids, uint32_t id_bytes, uint32_t n, uint8_t* buf,
                            size_t cap, uint64_t* offs, uint32_t* keep, uint32_t* n_out, uint64_t* need);
/* Id of an inserted filter, TM_ENOENT if absent. */
TM_API int  tm_filter_id(tm_engine* e, const uint8_t* filter, size_t len, uint32_t* id);

/* ---- emqx_topic (src/emqx_topic.erl), host predicates ----------------- */
/* emqx_topic:match/2 (:65-87) on binaries: 1 match, 0 no match. */
TM_API int  tm_topic_match(const uint8_t* name, size_t name_len, const uint8_t* filter, size_t filter_len);
/* emqx_topic:wildcard/1 (:52-62). */
TM_API int  tm_topic_wildcard(const uint8_t* topic, size_t len);
/* emqx_topic:validate/2 (:96-127): 0 ok, TM_EINVAL otherwise; *reason set to
 * one of "empty_topic", "topic_too_long", "topic_invalid_#",
 * "topic_invalid_char", "topic_name_error". */
TM_API int  tm_topic_validate(int is_name, const uint8_t* topic, size_t len, const char** reason);

/* Batched predicate on the device: emqx_topic:match(Name_i, Rule_j) for n
 * names x r rule filters -- the pairwise callers that do not use the trie:
 * ACL rules (src/emqx_access_rule.erl:124-139, word-list form: dollar_rule = 0),
 * rewrite rules (src/emqx_mod_rewrite.erl:86-90) and topic tracers
 * (src/emqx_tracer.erl:142-151), both binary form: dollar_rule = 1 (a name
 * starting with '$' never matches a filter starting with '+' or '#',
 * src/emqx_topic.erl:68-71).  bits (host memory, n * ceil(r/32) u32): bit j%32
 * of word i*ceil(r/32) + j/32 = match(name i, rule j). */
TM_API int  tm_rules_match(tm_engine* e, const uint8_t* names, const uint64_t* name_offsets, uint32_t n,
                           const uint8_t* rules, const uint64_t* rule_offsets, uint32_t r, int dollar_rule,
                           uint32_t* bits);

/* ---- ACL check: emqx_access_control:check_acl/3 on the device ---------- */
/* A batch of (client, access, topic) requests against one ordered rule list:
 * emqx_mod_acl_internal:check_acl/5 (src/emqx_mod_acl_internal.erl:69-121)
 * over compiled emqx_access_rule rules (src/emqx_access_rule.erl:43-154) --
 * the who clause, the publish/subscribe split as a per-rule mask, pattern
 * filters (a %c / %u level takes the client's id / name as ONE word that is
 * never an atom; an undefined field leaves the level a literal), {eq, T}
 * filters (byte equality), emqx_topic:match/2 in its word-list form (no '$'
 * rule, src/emqx_topic.erl:74-87) and the first-match-wins fold.  One kernel,
 * from the raw topic bytes; nothing is tokenised on the host. */
#define TM_ACL_DENY      0u
#define TM_ACL_ALLOW     1u
#define TM_ACL_NOMATCH   2u      /* verdict only: falls to the zone's acl_nomatch */
#define TM_ACL_PUBLISH   1u      /* request access, and rule access: */
#define TM_ACL_SUBSCRIBE 2u
#define TM_ACL_PUBSUB    3u      /* rules only; rule access 0 = {A, all} (who and topics ignored) */
#define TM_WHO_ALL        0u
#define TM_WHO_CLIENT_ALL 1u
#define TM_WHO_USER_ALL   2u
#define TM_WHO_CLIENT     3u
#define TM_WHO_USER       4u
#define TM_WHO_IPADDR     5u
#define TM_WHO_AND        6u
#define TM_WHO_OR         7u
#define TM_ACL_MAX_WHO_DEPTH 32u  /* a leaf is depth 1, 'and' / 'or' 1 + its deepest child */
/* A who expression as a pre-order node array: AND / OR carry the count of
 * their direct children, which follow (each with its own subtree). */
typedef struct {
    uint32_t       kind;         /* TM_WHO_* */
    uint32_t       n_children;   /* AND / OR */
    const uint8_t* val;          /* CLIENT / USER: the binary */
    uint32_t       val_len;
    uint8_t        family;       /* IPADDR: 4 | 6 */
    uint8_t        lo[16];       /* IPADDR: inclusive range, network order (IPv4 in the first 4 bytes) */
    uint8_t        hi[16];
} tm_acl_who;
typedef struct {
    const uint8_t* filter;
    uint32_t       len;          /* <= TM_MAX_TOPIC_LEN */
    uint32_t       eq;           /* 1: {eq, Topic} -- literal, no pattern */
} tm_acl_topic;
typedef struct {
    uint32_t            allow;     /* TM_ACL_DENY | TM_ACL_ALLOW */
    uint32_t            access;    /* 0 | TM_ACL_PUBLISH | TM_ACL_SUBSCRIBE | TM_ACL_PUBSUB */
    const tm_acl_who*   who;
    uint32_t            n_who;     /* nodes of the who array (exactly one tree) */
    const tm_acl_topic* topics;
    uint32_t            n_topics;  /* 0: the rule never matches (src/emqx_access_rule.erl:126-127) */
} tm_acl_rule;
typedef struct {
    uint32_t        m;
    const uint8_t*  clientids;         /* concatenated */
    const uint64_t* clientid_offsets;  /* m + 1 */
    const uint8_t*  usernames;
    const uint64_t* username_offsets;  /* m + 1 */
    const uint8_t*  flags;             /* m: bit 0 clientid defined, bit 1 username defined */
    const uint8_t*  family;            /* m: 0 peerhost undefined | 4 | 6 */
    const uint8_t*  peerhost;          /* 16 B per client, network order (IPv4 in the first 4 bytes) */
} tm_acl_clients;
typedef struct tm_acl tm_acl;
/* Compiles the n rules on the host into one flat block (rule table, who
 * programs in postfix form, filter bytes with per-level kinds) and uploads it
 * to every replica of the engine; the handle is immutable (a reload creates a
 * new one and frees the old; no lock is shared with the trie) and must be
 * freed before the engine is destroyed.  Works on a host-only engine (no
 * upload).  TM_EINVAL + tm_last_error(): allow > 1, access > 3, a who array
 * that is not exactly one tree, who nesting deeper than TM_ACL_MAX_WHO_DEPTH
 * (the device evaluates who over a 32-bit stack), an unknown who kind, an
 * IPADDR family other than 4 / 6, a filter longer than TM_MAX_TOPIC_LEN. */
TM_API int  tm_acl_create(tm_engine* e, const tm_acl_rule* rules, uint32_t n, tm_acl** out);
TM_API void tm_acl_free(tm_engine* e, tm_acl* acl);
/* Request i = (clients[client_of[i]], access[i], topic i); topics / offsets as
 * in tm_match_batch.  verdict[i] = TM_ACL_ALLOW / _DENY / _NOMATCH, rule[i] =
 * index of the deciding rule in the list given to tm_acl_create, TM_NONE on
 * nomatch.  TM_EINVAL + tm_last_error(): a name longer than TM_MAX_TOPIC_LEN,
 * client_of[i] >= m, access[i] not TM_ACL_PUBLISH / TM_ACL_SUBSCRIBE, a
 * client family not 0 / 4 / 6.  TM_ENODEV on a host-only engine.  On an
 * engine with several replicas a batch of 65,536+ requests is split over them. */
TM_API int  tm_acl_check(tm_engine* e, tm_acl* acl, const tm_acl_clients* clients, const uint8_t* topics,
                         const uint64_t* offsets, const uint32_t* client_of, const uint8_t* access, uint32_t n,
                         uint8_t* verdict, uint32_t* rule);
/* Device time (HIP events) of the kernel of the last tm_acl_check on this
 * handle, the slowest slice of a split batch; 0 before the first. */
TM_API float tm_acl_kernel_ms(tm_engine* e, tm_acl* acl);

/* ---- replicated multi-device group (BASELINE config C3) --------------- */
/* A view of one tm_create_replicated engine (tm_group_engine(g, i) returns it
 * for every i < tm_group_size): one host trie, one HBM replica per listed
 * device (a device may be listed twice: two replicas on one GPU), so node /
 * filter ids are identical everywhere (the reference replicates emqx_trie to
 * every node, src/emqx_trie.erl:53-74).  The split form keeps one slice per
 * replica explicit: a publish batch is split into contiguous slices matched
 * concurrently with no collective, and the slices' CSRs concatenate into the
 * batch's CSR. */
typedef struct tm_group tm_group;
typedef struct tm_group_batch tm_group_batch;
TM_API int  tm_group_create(const int32_t* devices, uint32_t n_devices, const tm_config* cfg, tm_group** out);
TM_API void tm_group_destroy(tm_group* g);
TM_API uint32_t tm_group_size(tm_group* g);
/* Replica i (read-only use: stats, filter bytes; mutate only through tm_group_*). */
TM_API tm_engine* tm_group_engine(tm_group* g, uint32_t i);
TM_API int  tm_group_trie_insert(tm_group* g, const uint8_t* topic, size_t len);
TM_API int  tm_group_trie_delete(tm_group* g, const uint8_t* topic, size_t len);
TM_API int  tm_group_insert_many(tm_group* g, const uint8_t* filters, const uint64_t* offsets, uint32_t n,
                                 uint64_t* n_inserted);
TM_API int  tm_group_route_apply(tm_group* g, const uint8_t* topics, const uint64_t* offsets, const uint32_t* dests,
                                 const uint8_t* ops, uint32_t n, uint64_t* n_changed);
TM_API int  tm_group_sync(tm_group* g);
/* Split form: prepare slices (H2D on every device), launch all (async), wait
 * all, merged CSR (group-owned pinned memory, valid until the batch is
 * re-prepared or freed).  A non-NULL *out is re-prepared in place. */
TM_API int  tm_group_prepare(tm_group* g, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                             tm_group_batch** out);
TM_API int  tm_group_launch(tm_group* g, tm_group_batch* b);
TM_API int  tm_group_wait(tm_group* g, tm_group_batch* b);
TM_API int  tm_group_result(tm_group* g, tm_group_batch* b, tm_result* out);
/* tm_batch_sample over a group batch: publishes[0..k) (indices into the whole
 * batch, any order) -> their rows as a host CSR in that order, each gathered
 * on the device of the slice that holds it (group-owned memory, valid until
 * the next tm_group_sample or free of the batch). */
TM_API int  tm_group_sample(tm_group* g, tm_group_batch* b, const uint32_t* publishes, uint32_t k, tm_result* out);
/* Counters summed over the slices; ms_match / ms_total = the slowest slice. */
TM_API int  tm_group_batch_stats(tm_group* g, tm_group_batch* b, tm_batch_stats* out);
TM_API void tm_group_batch_free(tm_group* g, tm_group_batch* b);
/* prepare + launch + wait + result in one call. */
TM_API int  tm_group_match_batch(tm_group* g, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                                 tm_result* out);
/* Deliveries of a waited group batch (tm_batch_dispatch per slice, merged in
 * publish order into group-owned memory valid like tm_group_result's). */
TM_API int  tm_group_dispatch(tm_group* g, tm_group_batch* b, tm_deliveries* out);
/* The per-publish and whole-batch calls of the group's engine (each spans the
 * replicas, see tm_create_replicated): tm_match_async, tm_match_coalesced,
 * tm_match_routes_batch, tm_rules_match. */
TM_API int  tm_group_match_async(tm_group* g, const uint8_t* topic, size_t len, tm_match_cb cb, void* ctx);
TM_API int  tm_group_match_coalesced(tm_group* g, const uint8_t* topic, size_t len, uint32_t* ids, uint32_t cap,
                                     uint32_t* n_out);
TM_API int  tm_group_match_routes_batch(tm_group* g, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                                        tm_routes* out);
TM_API int  tm_group_rules_match(tm_group* g, const uint8_t* names, const uint64_t* name_offsets, uint32_t n,
                                 const uint8_t* rules, const uint64_t* rule_offsets, uint32_t r, int dollar_rule,
                                 uint32_t* bits);

/* ---- filter-sharded group in one process (BASELINE config C4) -------- */
/* Subscription sets too large to replicate, partitioned over G shard engines
 * (one per listed device; a device may repeat), no collective: a filter whose
 * first two levels are literal lives on shard tm_filter_shard(); all others
 * are replicated on every shard.  A publish is matched completely by its
 * owner shard (the shard of its first two words, or any shard when only
 * replicated filters can match it), so rows stay bit-exact.  A batch is cut
 * into G contiguous slices, slice i tokenised on shard i's device at prepare.
 * One step: every slice partitioned by owner on its own device, every shard
 * receiving its parts (D2D, xGMI peer copies, or staged through pinned host
 * memory) and walking them -- all queued, then ONE host wait.  The rows stay
 * where each shard's walk wrote them; the publish-order CSR with global
 * filter ids (local id * G + shard) is built on request (tm_sharded_result /
 * tm_sharded_device_csr).  The shards' dictionaries grow only by the deltas of
 * tm_sharded_insert_many, so word ids agree everywhere.  Reference: the
 * replicated emqx_trie (src/emqx_trie.erl:53-74) matched in full by
 * match_routes/1 (src/emqx_router.erl:127-141); sharding it is new. */
typedef struct tm_sharded tm_sharded;
typedef struct tm_sharded_batch tm_sharded_batch;
typedef struct {
    tm_batch_stats match;     /* summed over the parts; ms_* = the slowest part */
    float ms_partition;       /* device time: owner + partition of a slice (the slowest) */
    float ms_exchange;        /* device time: a shard receiving its parts (the slowest) */
    float ms_step;            /* host wall time of the last tm_sharded_run */
    float ms_unpartition;     /* host wall time: the publish-order CSR (on request) */
    uint32_t host_waits;      /* blocking host waits in the last step: 1, + 1 per capacity relaunch */
    uint32_t part_topics[64]; /* publishes each shard matched */
    float ms_stage;           /* host wall time of the last prepare's copy of the publishes into pinned memory */
    float ms_plan;            /* host wall time of the last prepare's plan (uploads, device tokenisers, counts);
                                 the uploads start while the copy runs, so the two overlap */
} tm_sharded_stats;
/* how shard i's memory reaches shard j's device */
#define TM_LINK_SAME   0      /* same device: D2D copies */
#define TM_LINK_PEER   1      /* peer access enabled both ways (xGMI): peer copies */
#define TM_LINK_STAGED 2      /* no peer access: copies staged through pinned host memory */
TM_API int  tm_sharded_create(const int32_t* devices, uint32_t n_shards, const tm_config* cfg, tm_sharded** out);
TM_API void tm_sharded_destroy(tm_sharded* s);
TM_API uint32_t tm_sharded_size(tm_sharded* s);
/* TM_LINK_* between shards i and j (TM_EINVAL out of range). */
TM_API int  tm_sharded_link(tm_sharded* s, uint32_t i, uint32_t j);
/* Shard g's engine (read-only use: stats, filter bytes of its local ids). */
TM_API tm_engine* tm_sharded_engine(tm_sharded* s, uint32_t shard);
/* Interns n words in order on every shard (tm_dict_load). */
TM_API int  tm_sharded_dict_load(tm_sharded* s, const uint8_t* words, const uint64_t* offsets, uint32_t n);
/* emqx_trie:insert/1 of a subscribe batch: the batch's literal words no shard
 * knows are appended to every shard's dictionary in first-appearance order,
 * then every shard inserts its filters and the replicated ones.
 * *n_inserted = insertions summed over the shards. */
TM_API int  tm_sharded_insert_many(tm_sharded* s, const uint8_t* filters, const uint64_t* offsets, uint32_t n,
                                   uint64_t* n_inserted);
/* emqx_trie:delete/1 of an unsubscribe batch on every shard (absent: no-op).
 * *n_deleted = deletions summed over the shards each filter lives on (its
 * owner, or all G for a replicated filter), as tm_sharded_insert_many counts. */
TM_API int  tm_sharded_delete_many(tm_sharded* s, const uint8_t* filters, const uint64_t* offsets, uint32_t n,
                                   uint64_t* n_deleted);
/* A publish batch: bytes copied (into pinned memory, by several threads),
 * slice i tokenised on shard i's device and its parts counted (the plan of
 * the exchange).  A non-NULL *out is re-prepared in place. */
TM_API int  tm_sharded_prepare(tm_sharded* s, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                               tm_sharded_batch** out);
/* One step (returns with every shard's rows in its HBM; one host wait). */
TM_API int  tm_sharded_run(tm_sharded* s, tm_sharded_batch* b);
/* D2H of the step's CSR of global filter ids (memory valid like tm_result). */
TM_API int  tm_sharded_result(tm_sharded* s, tm_sharded_batch* b, tm_result* out);
TM_API int  tm_sharded_device_csr(tm_sharded* s, tm_sharded_batch* b, const uint32_t** d_row_offsets,
                                  const uint32_t** d_ids, uint64_t* n_matches);
TM_API int  tm_sharded_batch_stats(tm_sharded* s, tm_sharded_batch* b, tm_sharded_stats* out);
TM_API void tm_sharded_batch_free(tm_sharded* s, tm_sharded_batch* b);
/* prepare + run + result in one call. */
TM_API int  tm_sharded_match_batch(tm_sharded* s, const uint8_t* topics, const uint64_t* offsets, uint32_t n,
                                   tm_result* out);
/* Bytes of global filter id gid (tm_filter_copy on its shard). */
TM_API int  tm_sharded_filter_copy(tm_sharded* s, uint32_t gid, uint8_t* buf, size_t cap, size_t* len);

/* ---- diagnostics ------------------------------------------------------ */
/* Consistency check of the host edge hash (tests): slots of a bucket filled
 * in order, every key's probe run unbroken and within max_disp, every key
 * found by the lookup the kernels mirror.  TM_EIO + tm_last_error() on the
 * first violation; *max_disp_out (may be NULL) = the largest displacement.
 * A largest displacement above the probe bound (48 buckets, MAX_PROBE_DISP)
 * is a violation too, reported last: *max_disp_out is set all the same.
 * (An insert re-packs into twice the buckets, up to four times, until the
 * bound holds; one that still cannot meet it returns TM_EOVERFLOW +
 * tm_last_error(), its filter stays in the trie, and launches return
 * TM_EOVERFLOW until a later insert or re-pack has restored the bound.) */
TM_API int  tm_debug_check(tm_engine* e, uint64_t* max_disp_out);
/* The host edge hash as it is stored (tests; read-only): *nbuckets_out = its
 * bucket count (four 16-B slots each); the slots are copied to out as four
 * u32 each -- parent, word, child, hash, flag and signature bits included, a
 * free slot's parent 0xFFFFFFFF -- when cap_slots >= 4 * *nbuckets_out, else
 * TM_EOVERFLOW (the bucket count is set all the same: call with out = NULL,
 * cap_slots = 0 to size the buffer).  Works on a host-only engine. */
TM_API int  tm_debug_slots(tm_engine* e, uint32_t* out, uint64_t cap_slots, uint64_t* nbuckets_out);
/* The fan-out's width limit (tests): a scan block of tm_batch_dispatch that
 * delivers more keeps its match offsets as u64.  2^32 - 1 unless TM_FAN_BIG
 * was set when the engine was created; 0 then means every block that has a
 * delivery. */
TM_API uint64_t tm_debug_fan_big_limit(tm_engine* e);
/* The generic path of a batch (tests): out = {walks of the last launch that
 * outgrew the LDS probe stack and started again in global scratch, probe
 * stack entries and row entries of a wave's global scratch (both grow 4x when
 * a row exceeds them, and the batch is launched again), waves}.  The first is
 * 0 until tm_batch_wait has returned. */
TM_API int  tm_debug_batch_slow(tm_batch* b, uint32_t out[4]);
/* The delta-upload path (tests).  tm_sync / a launch bring every replica's
 * copy of the edge hash, the filter metadata and bytes and the word dictionary
 * up to the host trie in three stages: gather (the re-pack decision, the dirty
 * slots / filter nodes / dictionary keys staged once, full-or-delta decided),
 * per-replica apply (copies and scatter kernels), consume (dirty sets
 * emptied).  The three calls below look at that path from outside.
 *
 * tm_debug_upload_info: what is pending and what the path has done so far,
 * read under the engine lock; uploads nothing.  out[TM_UPLOAD_*]; the counters
 * count per replica applied to (the shadow below counts as one). */
enum {
    TM_UPLOAD_SLOTS = 0,        /* edge-hash slots on the host */
    TM_UPLOAD_DIRTY,            /* slots listed for the next delta */
    TM_UPLOAD_FULL_DIRTY,       /* 1: the next upload copies the whole edge hash */
    TM_UPLOAD_DIRTY_F,          /* filter-metadata nodes listed for the next delta */
    TM_UPLOAD_FULL_F_DIRTY,     /* 1: the next upload copies all filter metadata */
    TM_UPLOAD_NODES,            /* node records (live or not) */
    TM_UPLOAD_FBYTES,           /* bytes in the filter arena */
    TM_UPLOAD_DICT_KEYS,        /* slots of the dictionary's key table */
    TM_UPLOAD_DICT_DIRTY,       /* key slots listed for the next delta (a slot may be listed twice) */
    TM_UPLOAD_DICT_GEN,         /* rebuilds of the key table */
    TM_UPLOAD_DICT_TAILS,       /* dictionary tails */
    TM_UPLOAD_DICT_ARENA,       /* bytes in the word arena */
    TM_UPLOAD_NEEDS_REPACK,     /* 1: the next upload re-packs the edge hash first */
    TM_UPLOAD_N_REPACKS,        /* counters from here on: re-packs */
    TM_UPLOAD_N_FMETA_FULL,     /* filter metadata copied whole */
    TM_UPLOAD_N_FMETA_DELTA,    /* ... scattered */
    TM_UPLOAD_N_FMETA_NODES,    /* nodes in those scatters */
    TM_UPLOAD_N_KEYS_FULL,      /* dictionary keys copied whole */
    TM_UPLOAD_N_KEYS_DELTA,     /* ... scattered */
    TM_UPLOAD_N_KEYS_SCATTERED, /* key slots in those scatters */
    TM_UPLOAD_N_TAIL_PINNED,    /* appended tails copied through the pinned staging */
    TM_UPLOAD_N_TAIL_PAGEABLE,  /* ... from pageable memory */
    TM_UPLOAD_N_SLOTS_REALLOC,  /* edge-hash buffers (re)allocated */
    TM_UPLOAD_N_FULL,           /* tm_engine_stats uploads_full / uploads_delta / delta_slots */
    TM_UPLOAD_N_DELTA,
    TM_UPLOAD_N_DELTA_SLOTS,
    TM_UPLOAD_INFO_N
};
TM_API int  tm_debug_upload_info(tm_engine* e, uint64_t out[TM_UPLOAD_INFO_N]);
/* A table comparison: out[2 * t] = elements of table t that differ from the
 * host's over its live extent (every slot, every node record, the bytes in
 * use; an element the copy has no room for differs), out[2 * t + 1] = the first
 * such index, ~0 if none.  Filter metadata of nodes that are no filter now is
 * counted apart: it is never read, and only the other rows must be 0. */
enum {
    TM_DIFF_SLOTS = 0, TM_DIFF_FOFF, TM_DIFF_FLEN, TM_DIFF_FOFF_DEAD, TM_DIFF_FLEN_DEAD, TM_DIFF_FBYTES,
    TM_DIFF_DKEY, TM_DIFF_TAIL, TM_DIFF_ARENA, TM_DIFF_TABLES
};
/* tm_debug_shadow_sync (tests): the engine keeps a stand-in for a replica in
 * host memory, empty until the first call.  apply != 0: the gather stage runs,
 * its result is applied to the shadow as a replica would receive it (whole
 * copies where the gather or a size change says so, the staged index / value
 * pairs otherwise, the appended tails from the shadow's own marks, buffers
 * regrown by the replicas' rules and losing their contents), and the consume
 * stage runs.  Then, and alone with apply == 0, the shadow is compared with
 * the host tables.  Works on a host-only engine; covers which slots are
 * marked and which path is chosen, not the copies and scatter kernels.
 * TM_EINVAL with apply != 0 on an engine with replicas: the dirty sets are
 * consumed once. */
TM_API int  tm_debug_shadow_sync(tm_engine* e, int apply, uint64_t out[2 * TM_DIFF_TABLES]);
/* tm_debug_replica_diff (tests): with sync != 0 first what tm_sync does; then
 * the replica's seven tables are copied back and compared as above.  TM_EIO +
 * tm_last_error() if the replica's edge hash or dictionary key table has
 * another size than the host's; TM_ENODEV on a host-only engine. */
TM_API int  tm_debug_replica_diff(tm_engine* e, uint32_t replica, int sync, uint64_t out[2 * TM_DIFF_TABLES]);
/* Text of the last TM_EIO on this thread (HIP error string + call site). */
TM_API const char* tm_last_error(void);
TM_API const char* tm_build_info(void);
/* Number of visible HIP devices (0 when there is no driver or device). */
TM_API int  tm_device_count(void);

#ifdef __cplusplus
}
#endif
#endif /* EMQX_TM_H */
