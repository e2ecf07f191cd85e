// tm_upload.cpp -- delta uploads: the host trie's dirty nodes, edge slots and
// dictionary entries copied to every HBM replica before the next walk.
#include "tm_engine_impl.hpp"

bool tm_engine::upload_pending(const Replica& R) {
    if (full_dirty || !dirty.empty() || R.d_nslots != slots.size() || needs_repack()) return true;
    if (full_f_dirty || !dirty_f.empty() || fbytes.size() > R.fbytes_uploaded) return true;
    if (R.tab.d_foff.cap < nd.size() || R.tab.d_flen.cap < nd.size() || R.tab.d_fbytes.cap < fbytes.size() + 1)
        return true;
    if (dev_tok && (R.d_dict_n != dict.keys().size() || R.d_dict_gen != dict.gen() || !dict.dirty().empty() ||
                    dict.tails().size() > R.tails_uploaded || dict.arena().size() > R.arena_uploaded ||
                    R.tab.d_arena.cap < dict.arena().size() + 1))
        return true;
    return false;
}

int tm_engine::ensure_delta_idle() {
    for (Replica* R : reps)
        if (R->delta_inflight) {
            HIP_OK(hipSetDevice(R->device));
            HIP_OK(hipEventSynchronize(R->tab.ev_delta.e));
            R->delta_inflight = false;
        }
    return TM_OK;
}

int tm_engine::sync_device(const Replica* back) {
    if (reps.empty()) return TM_ENODEV;
    bool any = false;
    for (Replica* R : reps) any = any || upload_pending(*R);
    if (!any) {   // (an upload in flight is ordered before later work on the device: no host wait)
        HIP_OK(hipSetDevice(back ? back->device : device));
        return TM_OK;
    }
    // the last async upload still reads the pinned staging this one rewrites
    int rc = ensure_delta_idle();
    if (rc) return rc;
    Gather G;
    if ((rc = gather_deltas(G))) return rc;
    // apply to every replica (different devices run their copies concurrently)
    std::vector<uint8_t> pageable(reps.size(), 0), async(reps.size(), 0);
    for (size_t r = 0; r < reps.size(); ++r) {
        Replica& R = *reps[r];
        bool pg = false, as = false;
        if ((rc = upload_to(R, G.slots_full, G.keys_full, G.nn, pg, as))) return rc;
        pageable[r] = pg;
        async[r] = as;
    }
    if ((rc = consume_deltas(G, pageable, async))) return rc;
    HIP_OK(hipSetDevice(back ? back->device : device));
    return TM_OK;
}

int tm_engine::gather_deltas(Gather& G) {
    int rc;
    // staging: pinned for the replicas' copies; plain host memory on an engine
    // without a device (tm_debug_shadow_sync), where nothing can be pinned
    const bool host_only = reps.empty();
    // after a bulk build or heavy churn, re-pack the host table to the
    // target load so the walk's working set stays small (a full upload)
    if (needs_repack()) {
        rehash((size_t)(live_edges / target_load));
        if (!bound_probe_runs()) return probe_bound_error();   // (the re-packed table is what launches read)
        rebuild_lext();   // (a full upload follows the re-pack anyway)
        ++up_repacks;
    }
    G.nn = nd.size();
    // gather the deltas once
    const bool slots_full = G.slots_full = full_dirty || dirty.size() > slots.size() / 8;
    {   // the blob's layout: the slot deltas, then the filter-metadata deltas
        const size_t k1 = (!slots_full && !dirty.empty()) ? dirty.size() : 0;
        const size_t k2 = (!full_f_dirty && !dirty_f.empty()) ? dirty_f.size() : 0;
        auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
        blob_off[0] = 0;
        blob_off[1] = al(k1 * sizeof(uint32_t));
        blob_off[2] = blob_off[1] + al(k1 * sizeof(Slot));
        blob_off[3] = blob_off[2] + al(k2 * sizeof(uint32_t));
        blob_off[4] = blob_off[3] + al(k2 * sizeof(uint64_t));
        blob_bytes = blob_off[4] + al(k2 * sizeof(uint32_t));
        uint8_t* blob = nullptr;
        if (host_only) {
            shadow.blob.resize(blob_bytes / 8 + 1);   // (u64 elements: every part is 16-B aligned in the pinned blob, 8-B here)
            blob = reinterpret_cast<uint8_t*>(shadow.blob.data());
        } else {
            if (blob_bytes && (rc = h_dblob.reserve(blob_bytes))) return rc;
            blob = h_dblob.p;
        }
        h_didx = reinterpret_cast<uint32_t*>(blob + blob_off[0]);
        h_dval = reinterpret_cast<Slot*>(blob + blob_off[1]);
        h_fidx = reinterpret_cast<uint32_t*>(blob + blob_off[2]);
        h_foffv = reinterpret_cast<uint64_t*>(blob + blob_off[3]);
        h_flenv = reinterpret_cast<uint32_t*>(blob + blob_off[4]);
    }
    if (!slots_full && !dirty.empty()) {
        const size_t k = dirty.size();
        par_chunks(k, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i) {
                if (i + 16 < i1) __builtin_prefetch(&slots[dirty[i + 16]]);
                const uint32_t d = dirty[i];
                h_didx[i] = d;
                h_dval[i] = slots[d];
                // the set is consumed here (every set bit is in `dirty`; words
                // shared by two entries are cleared twice, to the same 0)
                __atomic_store_n(&dirty_mark[d >> 6], 0ull, __ATOMIC_RELAXED);
            }
        });
    }
    if (!full_f_dirty && !dirty_f.empty()) {
        const size_t k = dirty_f.size();
        par_chunks(k, [&](size_t i0, size_t i1) {
            for (size_t i = i0; i < i1; ++i) {
                const uint32_t c = dirty_f[i];
                h_fidx[i] = c; h_foffv[i] = n_foff[c]; h_flenv[i] = n_flen[c];
                dirty_f_mark[c] = 0;   // (each node is listed once)
            }
        });
    }
    std::vector<uint32_t>& dx = dict.dirty();
    const bool keys_full = G.keys_full = dx.size() > dict.keys().size() / 8;
    if (dev_tok && !keys_full && !dx.empty()) {
        std::sort(dx.begin(), dx.end());
        dx.erase(std::unique(dx.begin(), dx.end()), dx.end());   // a slot may move twice: scatter it once
        const size_t k = dx.size();
        uint32_t* xi;
        DictKey* xv;
        if (host_only) {
            shadow.dxidx.resize(k);
            shadow.dxval.resize(k);
            xi = shadow.dxidx.data();
            xv = shadow.dxval.data();
        } else {
            if ((rc = h_dxidx.reserve(k))) return rc;
            if ((rc = h_dxval.reserve(k))) return rc;
            xi = h_dxidx.p;
            xv = h_dxval.p;
        }
        for (size_t i = 0; i < k; ++i) {
            xi[i] = dx[i];
            xv[i] = dict.keys()[dx[i]];
        }
    }
    return TM_OK;
}

int tm_engine::consume_deltas(const Gather& G, const std::vector<uint8_t>& pageable, const std::vector<uint8_t>& async) {
    // the dirty sets are consumed: every replica has them now
    // (the delta gathers cleared their marks on the workers)
    if (G.slots_full) {
        full_dirty = false;
        for (uint32_t i : dirty) dirty_mark[i >> 6] = 0;   // every set bit is in `dirty`
        if (dirty_mark.size() != (slots.size() + 63) / 64) dirty_mark.assign((slots.size() + 63) / 64, 0);
    }
    dirty.clear();
    if (full_f_dirty) {
        full_f_dirty = false;
        dirty_f_mark.assign(G.nn, 0);
    }
    dirty_f.clear();
    if (dev_tok) dict.dirty().clear();
    for (size_t r = 0; r < reps.size(); ++r) {
        Replica& R = *reps[r];
        HIP_OK(hipSetDevice(R.device));
        if (pageable[r]) {
            // host vectors may be mutated / reallocated right after we return
            HIP_OK(hipStreamSynchronize(R.stream));
        } else if (async[r]) {
            HIP_OK(hipEventRecord(R.tab.ev_delta.e, R.stream));
            R.delta_inflight = true;
            if (!R.readers.empty()) {   // own-stream batches launched from now on wait for this upload
                HIP_OK(hipEventRecord(R.tab.ev_sync.e, R.stream));
                ++R.upload_seq;
            }
        }
    }
    return TM_OK;
}

int tm_engine::upload_to(Replica& R, bool slots_full, bool keys_full, size_t nn, bool& pageable_used, bool& async_used) {
    int rc;
    HIP_OK(hipSetDevice(R.device));
    const hipStream_t stream = R.stream;
    // tables change under the walks of this replica's own-stream batches in
    // flight: the uploads wait for them on the device, or on the host when
    // a table is reallocated (its old buffer is freed here)
    const bool realloc = R.d_nslots != slots.size() || R.tab.d_foff.cap < nn || R.tab.d_flen.cap < nn ||
                         R.tab.d_fbytes.cap < fbytes.size() + 1 ||
                         (dev_tok && (R.d_dict_n != dict.keys().size() || R.tab.d_tail.cap < dict.tails().size() + 1 ||
                                      R.tab.d_arena.cap < dict.arena().size() + 1));
    for (tm_batch* r : R.readers)
        if (r->launched && !r->done) {   // (a waited batch has finished reading them)
            if (realloc) {
                HIP_OK(hipStreamSynchronize(r->own));
                continue;
            }
            if ((rc = r->walk.ev_read.create(hipEventDisableTiming))) return rc;
            HIP_OK(hipEventRecord(r->walk.ev_read.e, r->own));
            HIP_OK(hipStreamWaitEvent(stream, r->walk.ev_read.e, 0));
        }
    // the delta blob, in one copy (the scatters below read their parts)
    if (blob_bytes) {
        if ((rc = R.tab.d_dblob.reserve(blob_bytes))) return rc;
        HIP_OK(hipMemcpyAsync(R.tab.d_dblob.p, h_dblob.p, blob_bytes, hipMemcpyHostToDevice, stream));
        async_used = true;
    }
    // edge hash
    bool full = slots_full;
    if (R.d_nslots != slots.size()) {
        R.tab.d_slots.reset();
        if ((rc = R.tab.d_slots.alloc(slots.size()))) return rc;
        R.d_nslots = slots.size();
        full = true;
        ++up_slots_realloc;
    }
    if (full) {
        pageable_used = true;
        HIP_OK(hipMemcpyAsync(R.tab.d_slots.p, slots.data(), slots.size() * sizeof(Slot), hipMemcpyHostToDevice,
                              stream));
        ++uploads_full;
    } else if (!dirty.empty()) {
        const size_t k = dirty.size();
        HIP_OK(launch_scatter_slots(R.tab.d_slots.p, reinterpret_cast<const uint32_t*>(R.tab.d_dblob.p + blob_off[0]),
                                    reinterpret_cast<const Slot*>(R.tab.d_dblob.p + blob_off[1]), (uint32_t)k, stream));
        ++uploads_delta;
        delta_slots += k;
        async_used = true;
    }
    // appended tails up to APP_MAX bytes in all go through the replica's
    // pinned staging (reserved once here: copies queued below read it until
    // the upload's event, and ensure_delta_idle waits for that before the
    // next upload reuses it)
    size_t app_need = 0, app_used = 0;
    {
        const uint64_t fb_from = R.tab.d_fbytes.cap < fbytes.size() + 1 ? 0 : R.fbytes_uploaded;
        app_need += fbytes.size() > fb_from ? fbytes.size() - fb_from : 0;
        if (dev_tok) {
            const size_t t_from = R.tab.d_tail.cap < dict.tails().size() + 1 ? 0 : R.tails_uploaded;
            const size_t a_from = R.tab.d_arena.cap < dict.arena().size() + 1 ? 0 : R.arena_uploaded;
            if (dict.tails().size() > t_from) app_need += (dict.tails().size() - t_from) * sizeof(DictTail) + 16;
            if (dict.arena().size() > a_from) app_need += dict.arena().size() - a_from + 16;
        }
    }
    const bool app_pinned = app_need > 0 && app_need <= APP_MAX;
    if (app_pinned && (rc = R.tab.h_app.reserve(app_need))) return rc;
    // a host range -> device, through the pinned staging when it fits
    auto h2d_tail = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        if (app_pinned && app_used + bytes <= R.tab.h_app.cap) {
            uint8_t* stg = R.tab.h_app.p + app_used;
            memcpy(stg, src, bytes);
            app_used = (app_used + bytes + 15) & ~(size_t)15;
            async_used = true;
            ++up_tail_pinned;
            return hipMemcpyAsync(dst, stg, bytes, hipMemcpyHostToDevice, stream);
        }
        pageable_used = true;
        ++up_tail_pageable;
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream);
    };
    // filter bytes (slow-path sort): arena + per-node (off, len)
    bool f_full = full_f_dirty;
    // (grown 2x: churn appends to these every step, and a new buffer
    // costs a full copy, a host wait for the batches reading the old one
    // and a new capture of every batch's launch graph -- its address is an
    // argument)
    if (R.tab.d_foff.cap < nn || R.tab.d_flen.cap < nn) {
        if ((rc = R.tab.d_foff.reserve(2 * nn))) return rc;
        if ((rc = R.tab.d_flen.reserve(2 * nn))) return rc;
        f_full = true;
    }
    if (R.tab.d_fbytes.cap < fbytes.size() + 1) {
        if ((rc = R.tab.d_fbytes.reserve(2 * (fbytes.size() + 1)))) return rc;
        R.fbytes_uploaded = 0;
    }
    if (fbytes.size() > R.fbytes_uploaded) {
        HIP_OK(h2d_tail(R.tab.d_fbytes.p + R.fbytes_uploaded, fbytes.data() + R.fbytes_uploaded,
                        fbytes.size() - R.fbytes_uploaded));
        R.fbytes_uploaded = fbytes.size();
    }
    if (f_full) {
        pageable_used = true;
        ++up_fmeta_full;
        HIP_OK(hipMemcpyAsync(R.tab.d_foff.p, n_foff.data(), nn * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(R.tab.d_flen.p, n_flen.data(), nn * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    } else if (!dirty_f.empty()) {
        const size_t k = dirty_f.size();
        const uint8_t* blob = R.tab.d_dblob.p;
        HIP_OK(launch_scatter_fmeta(R.tab.d_foff.p, R.tab.d_flen.p, reinterpret_cast<const uint32_t*>(blob + blob_off[2]),
                                    reinterpret_cast<const uint64_t*>(blob + blob_off[3]),
                                    reinterpret_cast<const uint32_t*>(blob + blob_off[4]), (uint32_t)k, stream));
        ++up_fmeta_delta;
        up_fmeta_nodes += k;
        async_used = true;
    }
    if (dev_tok && (rc = sync_dict(R, keys_full, pageable_used, async_used, h2d_tail))) return rc;
    return TM_OK;
}

// ------------------------------------------------------------ test hooks

// what upload_to + sync_dict would do to a replica, done to the shadow
void tm_engine::shadow_apply(const Gather& G) {
    Shadow& S = shadow;
    const size_t nn = G.nn;
    // edge hash
    bool full = G.slots_full;
    if (!S.slots_made || S.slots.size() != slots.size()) {
        Shadow::alloc(S.slots, slots.size());
        S.slots_made = true;
        full = true;
        ++up_slots_realloc;
    }
    if (full) {
        memcpy(static_cast<void*>(S.slots.data()), slots.data(), slots.size() * sizeof(Slot));
        ++uploads_full;
    } else if (!dirty.empty()) {
        const size_t k = dirty.size();
        for (size_t i = 0; i < k; ++i) S.slots[h_didx[i]] = h_dval[i];
        ++uploads_delta;
        delta_slots += k;
    }
    // (every appended tail counts as a pinned copy up to APP_MAX bytes in all, as upload_to sizes it)
    size_t app_need = 0;
    {
        const uint64_t fb_from = S.fbytes.size() < fbytes.size() + 1 ? 0 : S.fbytes_uploaded;
        app_need += fbytes.size() > fb_from ? fbytes.size() - fb_from : 0;
        if (dev_tok) {
            const size_t t_from = S.tail.size() < dict.tails().size() + 1 ? 0 : S.tails_uploaded;
            const size_t a_from = S.arena.size() < dict.arena().size() + 1 ? 0 : S.arena_uploaded;
            if (dict.tails().size() > t_from) app_need += (dict.tails().size() - t_from) * sizeof(DictTail) + 16;
            if (dict.arena().size() > a_from) app_need += dict.arena().size() - a_from + 16;
        }
    }
    const bool app_pinned = app_need > 0 && app_need <= APP_MAX;
    auto tail_copy = [&](void* dst, const void* src, size_t bytes) {
        memcpy(dst, src, bytes);
        ++(app_pinned ? up_tail_pinned : up_tail_pageable);
    };
    // filter bytes and per-node (off, len)
    bool f_full = full_f_dirty;
    if (S.foff.size() < nn || S.flen.size() < nn) {
        Shadow::reserve(S.foff, 2 * nn);
        Shadow::reserve(S.flen, 2 * nn);
        f_full = true;
    }
    if (S.fbytes.size() < fbytes.size() + 1) {
        Shadow::reserve(S.fbytes, 2 * (fbytes.size() + 1));
        S.fbytes_uploaded = 0;
    }
    if (fbytes.size() > S.fbytes_uploaded) {
        tail_copy(S.fbytes.data() + S.fbytes_uploaded, fbytes.data() + S.fbytes_uploaded, fbytes.size() - S.fbytes_uploaded);
        S.fbytes_uploaded = fbytes.size();
    }
    if (f_full) {
        memcpy(S.foff.data(), n_foff.data(), nn * sizeof(uint64_t));
        memcpy(S.flen.data(), n_flen.data(), nn * sizeof(uint32_t));
        ++up_fmeta_full;
    } else if (!dirty_f.empty()) {
        const size_t k = dirty_f.size();
        for (size_t i = 0; i < k; ++i) { S.foff[h_fidx[i]] = h_foffv[i]; S.flen[h_fidx[i]] = h_flenv[i]; }
        ++up_fmeta_delta;
        up_fmeta_nodes += k;
    }
    if (!dev_tok) return;
    // word dictionary
    const std::vector<DictKey>& tab = dict.keys();
    const std::vector<DictTail>& tl = dict.tails();
    const std::vector<uint8_t>& ar = dict.arena();
    const std::vector<uint32_t>& dx = dict.dirty();
    if (!S.dkey_made || S.dkey.size() != tab.size()) {
        Shadow::alloc(S.dkey, tab.size());
        S.dkey_made = true;
        S.dict_gen = ~0ull;
    }
    if (S.dict_gen != dict.gen() || G.keys_full) {
        memcpy(static_cast<void*>(S.dkey.data()), tab.data(), tab.size() * sizeof(DictKey));
        S.dict_gen = dict.gen();
        ++up_keys_full;
    } else if (!dx.empty()) {
        const size_t k = dx.size();
        for (size_t i = 0; i < k; ++i) S.dkey[S.dxidx[i]] = S.dxval[i];
        ++up_keys_delta;
        up_keys_scattered += k;
    }
    if (S.tail.size() < tl.size() + 1) {
        Shadow::reserve(S.tail, tl.size() + tl.size() / 2 + 64);
        S.tails_uploaded = 0;
    }
    if (tl.size() > S.tails_uploaded) {
        tail_copy(S.tail.data() + S.tails_uploaded, tl.data() + S.tails_uploaded,
                  (tl.size() - S.tails_uploaded) * sizeof(DictTail));
        S.tails_uploaded = tl.size();
    }
    if (S.arena.size() < ar.size() + 1) {
        Shadow::reserve(S.arena, ar.size() + 1);
        S.arena_uploaded = 0;
    }
    if (ar.size() > S.arena_uploaded) {
        tail_copy(S.arena.data() + S.arena_uploaded, ar.data() + S.arena_uploaded, ar.size() - S.arena_uploaded);
        S.arena_uploaded = ar.size();
    }
}

// out[2 * t] = elements of table t that differ from the host's over its live
// extent (elements the copy has no room for differ), out[2 * t + 1] = the
// first such index or ~0 (the TM_DIFF_* rows of emqx_tm.h)
void tm_engine::table_diff(const TableView& V, uint64_t* out) const {
    for (uint32_t t = 0; t < TM_DIFF_TABLES; ++t) { out[2 * t] = 0; out[2 * t + 1] = ~0ull; }
    auto note = [&](uint32_t t, size_t i) {
        if (!out[2 * t]++) out[2 * t + 1] = i;
    };
    for (size_t i = 0; i < slots.size(); ++i)
        if (i >= V.nslots || memcmp(&V.slots[i], &slots[i], sizeof(Slot)) != 0) note(TM_DIFF_SLOTS, i);
    for (size_t c = 0; c < nd.size(); ++c) {
        const bool is_filter = nd[c].live && nd[c].topic;
        if (c >= V.nfoff || V.foff[c] != n_foff[c]) note(is_filter ? TM_DIFF_FOFF : TM_DIFF_FOFF_DEAD, c);
        if (c >= V.nflen || V.flen[c] != n_flen[c]) note(is_filter ? TM_DIFF_FLEN : TM_DIFF_FLEN_DEAD, c);
    }
    for (size_t i = 0; i < fbytes.size(); ++i)
        if (i >= V.nfbytes || V.fbytes[i] != fbytes[i]) note(TM_DIFF_FBYTES, i);
    if (!dev_tok) return;
    const std::vector<DictKey>& tab = dict.keys();
    const std::vector<DictTail>& tl = dict.tails();
    const std::vector<uint8_t>& ar = dict.arena();
    for (size_t i = 0; i < tab.size(); ++i)
        if (i >= V.ndkey || memcmp(&V.dkey[i], &tab[i], sizeof(DictKey)) != 0) note(TM_DIFF_DKEY, i);
    for (size_t i = 0; i < tl.size(); ++i)
        if (i >= V.ntail || memcmp(&V.tail[i], &tl[i], sizeof(DictTail)) != 0) note(TM_DIFF_TAIL, i);
    for (size_t i = 0; i < ar.size(); ++i)
        if (i >= V.narena || V.arena[i] != ar[i]) note(TM_DIFF_ARENA, i);
}

extern "C" {

int tm_debug_upload_info(tm_engine* e, uint64_t out[TM_UPLOAD_INFO_N]) {
    if (!e || !out) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    const uint64_t v[TM_UPLOAD_INFO_N] = {
        e->slots.size(), e->dirty.size(), e->full_dirty,
        e->dirty_f.size(), e->full_f_dirty, e->nd.size(), e->fbytes.size(),
        e->dict.keys().size(), e->dict.dirty().size(), e->dict.gen(), e->dict.tails().size(), e->dict.arena().size(),
        e->needs_repack(),
        e->up_repacks, e->up_fmeta_full, e->up_fmeta_delta, e->up_fmeta_nodes, e->up_keys_full, e->up_keys_delta,
        e->up_keys_scattered, e->up_tail_pinned, e->up_tail_pageable, e->up_slots_realloc,
        e->uploads_full, e->uploads_delta, e->delta_slots};
    memcpy(out, v, sizeof v);
    return TM_OK;
}

int tm_debug_shadow_sync(tm_engine* e, int apply, uint64_t out[2 * TM_DIFF_TABLES]) {
    if (!e || !out) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    if (apply && !e->reps.empty()) return TM_EINVAL;   // the dirty sets are consumed once: by the replicas
    try {
        if (apply) {
            tm_engine::Gather G;
            int rc = e->gather_deltas(G);
            if (rc) return rc;
            e->shadow_apply(G);
            if ((rc = e->consume_deltas(G, {}, {}))) return rc;
        }
        const tm_engine::Shadow& S = e->shadow;
        const tm_engine::TableView V = {S.slots.data(), S.slots.size(), S.foff.data(), S.foff.size(),
                                        S.flen.data(),  S.flen.size(),  S.fbytes.data(), S.fbytes.size(),
                                        S.dkey.data(),  S.dkey.size(),  S.tail.data(), S.tail.size(),
                                        S.arena.data(), S.arena.size()};
        e->table_diff(V, out);
    } catch (...) {
        return TM_ENOMEM;
    }
    return TM_OK;
}

int tm_debug_replica_diff(tm_engine* e, uint32_t replica, int sync, uint64_t out[2 * TM_DIFF_TABLES]) {
    if (!e || !out) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    if (e->reps.empty()) return TM_ENODEV;
    if (replica >= e->reps.size()) return TM_EINVAL;
    int rc = e->set_device();
    if (rc) return rc;
    if (sync && (rc = e->sync_device())) return rc;
    for (Replica* R : e->reps) {   // (as tm_sync: every upload queued so far has landed)
        HIP_OK(hipSetDevice(R->device));
        HIP_OK(hipStreamSynchronize(R->stream));
        R->delta_inflight = false;
    }
    const Replica& R = *e->reps[replica];
    if (R.d_nslots != e->slots.size()) {
        snprintf(last_error(), 512, "replica %u holds %zu slots, the host %zu", replica, R.d_nslots, e->slots.size());
        (void)e->set_device();
        return TM_EIO;
    }
    if (e->dev_tok && R.d_dict_n != e->dict.keys().size()) {
        snprintf(last_error(), 512, "replica %u holds %zu dictionary slots, the host %zu", replica, R.d_dict_n,
                 e->dict.keys().size());
        (void)e->set_device();
        return TM_EIO;
    }
    try {
        // each table over the host's live extent, or as far as the replica's buffer goes
        HIP_OK(hipSetDevice(R.device));
        const size_t nn = e->nd.size();
        std::vector<Slot> sl(R.d_nslots);
        std::vector<uint64_t> fo(std::min(nn, R.tab.d_foff.cap));
        std::vector<uint32_t> fl(std::min(nn, R.tab.d_flen.cap));
        std::vector<uint8_t> fb(std::min(e->fbytes.size(), R.tab.d_fbytes.cap));
        std::vector<DictKey> dk(e->dev_tok ? R.d_dict_n : 0);
        std::vector<DictTail> dt(e->dev_tok ? std::min(e->dict.tails().size(), R.tab.d_tail.cap) : 0);
        std::vector<uint8_t> da(e->dev_tok ? std::min(e->dict.arena().size(), R.tab.d_arena.cap) : 0);
        auto back = [](void* dst, const void* src, size_t bytes) {
            return bytes ? hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) : hipSuccess;
        };
        HIP_OK(back(sl.data(), R.tab.d_slots.p, sl.size() * sizeof(Slot)));
        HIP_OK(back(fo.data(), R.tab.d_foff.p, fo.size() * sizeof(uint64_t)));
        HIP_OK(back(fl.data(), R.tab.d_flen.p, fl.size() * sizeof(uint32_t)));
        HIP_OK(back(fb.data(), R.tab.d_fbytes.p, fb.size()));
        HIP_OK(back(dk.data(), R.tab.d_dkey.p, dk.size() * sizeof(DictKey)));
        HIP_OK(back(dt.data(), R.tab.d_tail.p, dt.size() * sizeof(DictTail)));
        HIP_OK(back(da.data(), R.tab.d_arena.p, da.size()));
        const tm_engine::TableView V = {sl.data(), sl.size(), fo.data(), fo.size(), fl.data(), fl.size(), fb.data(),
                                        fb.size(), dk.data(), dk.size(), dt.data(), dt.size(), da.data(), da.size()};
        e->table_diff(V, out);
    } catch (...) {
        (void)e->set_device();
        return TM_ENOMEM;
    }
    return e->set_device();
}

}  // extern "C"
