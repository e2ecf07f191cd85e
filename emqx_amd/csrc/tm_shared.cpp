// tm_shared.cpp -- shared subscriptions (emqx_shared_sub): the group membership
// bag, its device tables with the round-robin cursors, and the batched
// dispatch (tm_batch_dispatch_shared).  Table layout in tm_internal.hpp.
#include "tm_engine_impl.hpp"

static_assert(SH_RANDOM == TM_SHARED_RANDOM && SH_ROUND_ROBIN == TM_SHARED_ROUND_ROBIN && SH_HASH == TM_SHARED_HASH,
              "the kernels' strategy codes are the ABI's");

namespace {

int einval(const char* msg) {
    snprintf(last_error(), 512, "%s", msg);
    return TM_EINVAL;
}

}  // namespace

int tm_engine::shared_subscribe(const uint8_t* t, size_t len, uint32_t group, uint32_t sub) {
    std::string k((const char*)t, len);
    auto it = shared_of.find(k);
    SharedRun* run = nullptr;
    if (it != shared_of.end())
        for (auto& r : it->second)
            if (r.group == group) { run = &r; break; }
    if (run && std::find(run->members.begin(), run->members.end(), sub) != run->members.end())
        return TM_OK;   // a bag stores an object once (:304)
    if (!run) {
        int rc = route_add(t, len, group);   // ets:member(?SHARED_SUBS, {Group, Topic}) = false (:299-302)
        if (rc) return rc;
        uint32_t slot;
        if (!shared_free.empty()) {
            slot = shared_free.back();
            shared_free.pop_back();
            ++shared_epoch[slot];
        } else {
            slot = (uint32_t)shared_epoch.size();
            shared_epoch.push_back(1u);
        }
        auto& runs = shared_of[k];
        runs.push_back(SharedRun{group, slot, {}});
        run = &runs.back();
        ++shared_runs;
    }
    run->members.push_back(sub);
    shared_topics_of[sub].emplace_back(std::move(k), group);
    ++shared_entries;
    shared_dirty = true;
    return TM_OK;
}

int tm_engine::shared_unsubscribe(const uint8_t* t, size_t len, uint32_t group, uint32_t sub) {
    std::string k((const char*)t, len);
    auto it = shared_of.find(k);
    if (it == shared_of.end()) return TM_ENOENT;
    auto& runs = it->second;
    size_t r = 0;
    while (r < runs.size() && runs[r].group != group) ++r;
    if (r == runs.size()) return TM_ENOENT;
    auto& mem = runs[r].members;
    auto mi = std::find(mem.begin(), mem.end(), sub);
    if (mi == mem.end()) return TM_ENOENT;   // delete_object of no record (:308-309)
    mem.erase(mi);
    --shared_entries;
    shared_dirty = true;
    auto ti = shared_topics_of.find(sub);
    if (ti != shared_topics_of.end()) {
        auto& ts = ti->second;
        auto e = std::find(ts.begin(), ts.end(), std::make_pair(k, group));
        if (e != ts.end()) ts.erase(e);
        if (ts.empty()) shared_topics_of.erase(ti);
    }
    if (mem.empty()) {   // the last member deletes the route (:310-313)
        shared_free.push_back(runs[r].slot);
        runs.erase(runs.begin() + (long)r);
        --shared_runs;
        if (runs.empty()) shared_of.erase(it);
        int rc = route_delete(t, len, group);
        if (rc && rc != TM_ENOENT) return rc;
    }
    return TM_OK;
}

int tm_engine::shared_member_down(uint32_t sub, uint64_t* n_removed) {
    uint64_t n = 0;
    auto it = shared_topics_of.find(sub);
    if (it != shared_topics_of.end()) {
        const std::vector<std::pair<std::string, uint32_t>> ts = it->second;
        for (const auto& kg : ts) {
            int rc = shared_unsubscribe((const uint8_t*)kg.first.data(), kg.first.size(), kg.second, sub);
            if (rc) return rc;
            ++n;
        }
    }
    if (n_removed) *n_removed = n;
    return TM_OK;
}

int tm_engine::shared_members(const uint8_t* t, size_t len, uint32_t group, uint32_t* buf, uint32_t cap, uint32_t* n) {
    *n = 0;
    auto it = shared_of.find(std::string((const char*)t, len));
    if (it == shared_of.end()) return TM_OK;
    for (const auto& r : it->second) {
        if (r.group != group) continue;
        *n = (uint32_t)r.members.size();
        std::copy_n(r.members.begin(), std::min<size_t>(cap, r.members.size()), buf);
        break;
    }
    return TM_OK;
}

int tm_engine::sync_shared(Replica& R) {
    const size_t nn = nd.size();
    if (shared_dirty || shared_version != version || shared_nn != nn || h_goff.empty()) {
        h_goff.assign(nn + 1, 0);
        std::vector<std::pair<uint32_t, const std::vector<SharedRun>*>> at;
        at.reserve(shared_of.size());
        h_gupd.resize(shared_epoch.size());
        for (size_t s = 0; s < shared_epoch.size(); ++s) h_gupd[s] = make_uint2(0u, shared_epoch[s]);
        for (const auto& kv : shared_of) {
            for (const auto& r : kv.second) h_gupd[r.slot].x = (uint32_t)r.members.size();
            const uint32_t n = node_of((const uint8_t*)kv.first.data(), kv.first.size());
            if (n == NONE || n >= nn) continue;   // not in the trie: no route, no dispatch
            at.emplace_back(n, &kv.second);
            h_goff[n + 1] += (uint32_t)kv.second.size();
        }
        for (size_t i = 0; i < nn; ++i) h_goff[i + 1] += h_goff[i];
        h_gruns.assign(h_goff[nn], make_uint4(0u, 0u, 0u, 0u));
        h_gmem.clear();
        h_gmem.reserve(shared_entries);
        for (const auto& a : at) {
            uint32_t k = h_goff[a.first];
            for (const auto& r : *a.second) {
                h_gruns[k++] = make_uint4(r.group, (uint32_t)h_gmem.size(), (uint32_t)r.members.size(), r.slot);
                h_gmem.insert(h_gmem.end(), r.members.begin(), r.members.end());
            }
        }
        h_gcnt.resize(std::max<size_t>(nn, 1));
        for (size_t i = 0; i < nn; ++i) h_gcnt[i] = (uint8_t)std::min<uint32_t>(h_goff[i + 1] - h_goff[i], 255u);
        shared_dirty = false;
        shared_version = version;
        shared_nn = (uint32_t)nn;
        ++shared_gen;
    }
    if (R.shared_gen == shared_gen) return TM_OK;
    const size_t sn = shared_nn, ns = h_gupd.size();
    int rc;
    if ((rc = dev_reserve(R.d_goff, R.c_goff, sn + 1))) return rc;
    if ((rc = dev_reserve(R.d_gcnt, R.c_gcnt, std::max<size_t>(sn, 1)))) return rc;
    if ((rc = dev_reserve(R.d_gruns, R.c_gruns, std::max<size_t>(h_gruns.size(), 1)))) return rc;
    if ((rc = dev_reserve(R.d_gmem, R.c_gmem, std::max<size_t>(h_gmem.size(), 1)))) return rc;
    if ((rc = dev_reserve(R.d_gupd, R.c_gupd, std::max<size_t>(ns, 1)))) return rc;
    if (ns > R.c_gslots || !R.d_gslots) {   // grown with the cursors kept; new slots start zeroed (epoch 0: never owned)
        const size_t old = R.d_gslots ? R.c_gslots : 0;
        if ((rc = dev_reserve(R.d_gslots, R.c_gslots, std::max<size_t>(ns, 1), true, old))) return rc;
        HIP_OK(hipMemsetAsync(R.d_gslots + old, 0, (R.c_gslots - old) * sizeof(SharedSlot), R.stream));
    }
    HIP_OK(hipMemcpyAsync(R.d_goff, h_goff.data(), (sn + 1) * 4, hipMemcpyHostToDevice, R.stream));
    if (sn) HIP_OK(hipMemcpyAsync(R.d_gcnt, h_gcnt.data(), sn, hipMemcpyHostToDevice, R.stream));
    if (!h_gruns.empty())
        HIP_OK(hipMemcpyAsync(R.d_gruns, h_gruns.data(), h_gruns.size() * sizeof(uint4), hipMemcpyHostToDevice,
                              R.stream));
    if (!h_gmem.empty())
        HIP_OK(hipMemcpyAsync(R.d_gmem, h_gmem.data(), h_gmem.size() * 4, hipMemcpyHostToDevice, R.stream));
    if (ns) {
        HIP_OK(hipMemcpyAsync(R.d_gupd, h_gupd.data(), ns * sizeof(uint2), hipMemcpyHostToDevice, R.stream));
        HIP_OK(launch_shared_fold(R.d_gslots, R.d_gupd, (uint32_t)ns, R.stream));
    }
    HIP_OK(hipStreamSynchronize(R.stream));
    R.shared_gen = shared_gen;
    return TM_OK;
}

int tm_engine::batch_dispatch_shared(tm_batch* b, const tm_shared_opts* o, tm_shared_deliveries* out) {
    if (!b->done) return einval("tm_batch_dispatch_shared: the batch has not been waited for");
    if (b->dedup) return einval("tm_batch_dispatch_shared: a TM_BATCH_DEDUP batch (the pick is per publish)");
    const bool counts_only = o->flags & TM_SHARED_COUNT_ONLY;
    const uint32_t n = b->n;
    Replica& R = *b->rep;
    const hipStream_t stream = R.stream;
    int rc;
    if ((rc = ensure_dense(b))) return rc;
    if ((rc = sync_shared(R))) return rc;
    const size_t nn = std::max<size_t>(n, 1);
    const uint64_t m64 = b->total;   // match entries (< 2^32: u32 result CSR)
    if (m64 > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    const uint32_t m = (uint32_t)m64;
    if ((rc = dev_reserve(b->d_gcount, b->c_gcount, (size_t)m + 1))) return rc;
    if ((rc = dev_reserve(b->d_geoff, b->c_geoff, (size_t)m + 1))) return rc;
    if ((rc = dev_reserve(b->d_grow, b->c_grow, nn + 1))) return rc;
    if ((rc = dev_reserve(b->d_gbsums, b->c_gbsums, (size_t)scan_block_count(m) + 1))) return rc;
    if ((rc = dev_reserve(b->d_gtotal, b->c_gtotal, 1))) return rc;
    if ((rc = dev_reserve(b->d_gtot64, b->c_gtot64, 1))) return rc;
    if ((rc = host_reserve(b->h_gtot64, b->ch_gtot64, 1))) return rc;
    for (hipEvent_t& ev : b->gev)
        if (!ev) HIP_OK(hipEventCreate(&ev));
    SharedArgs a{};
    a.row_off = b->d_rowoff; a.ids = b->d_ids; a.n = n; a.m = m;
    a.gcnt = R.d_gcnt; a.goff = R.d_goff; a.runs = R.d_gruns; a.mem = R.d_gmem;
    a.nnodes = shared_nn; a.nruns = (uint32_t)h_gruns.size(); a.nmem = (uint32_t)h_gmem.size();
    a.nslots = (uint32_t)h_gupd.size(); a.slots = R.d_gslots;
    a.ecount = b->d_gcount; a.eoff = b->d_geoff; a.bsums = b->d_gbsums; a.total = b->d_gtotal;
    a.total64 = b->d_gtot64; a.g_rowoff = b->d_grow;
    a.strategy = o->strategy; a.seed = o->seed;
    HIP_OK(hipEventRecord(b->gev[0], stream));
    HIP_OK(hipMemsetAsync(b->d_gtot64, 0, 8, stream));
    HIP_OK(launch_shared_count(a, stream));
    ScanArgs sa{};
    sa.count = b->d_gcount; sa.row_off = b->d_geoff; sa.block_sums = b->d_gbsums; sa.n = m;
    if (m) {
        HIP_OK(launch_scan(sa, stream, b->d_gtotal));
    } else {
        HIP_OK(hipMemsetAsync(b->d_gtotal, 0, 4, stream));
    }
    HIP_OK(launch_shared_rows(a, stream));
    HIP_OK(hipEventRecord(b->gev[1], stream));
    HIP_OK(hipMemcpyAsync(b->h_gtot64, b->d_gtot64, 8, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    const uint64_t total = b->h_gtot64[0];
    if (total > 0xFFFFFFF0ull) return TM_EOVERFLOW;   // the u32 scan wrapped: nothing of it is used
    float ms = 0.f, ms2 = 0.f;
    if (!counts_only) {
        if ((rc = dev_reserve(b->d_gfid, b->c_gfid, std::max<uint64_t>(total, 1)))) return rc;
        if ((rc = dev_reserve(b->d_ggrp, b->c_ggrp, std::max<uint64_t>(total, 1)))) return rc;
        if ((rc = dev_reserve(b->d_gsub, b->c_gsub, std::max<uint64_t>(total, 1)))) return rc;
        if (o->strategy == TM_SHARED_HASH && n) {
            if ((rc = dev_reserve(b->d_gkeys, b->c_gkeys, nn))) return rc;
            if ((rc = host_reserve(b->h_gkeys, b->ch_gkeys, nn))) return rc;
            memcpy(b->h_gkeys, o->keys, (size_t)n * 4);
            HIP_OK(hipMemcpyAsync(b->d_gkeys, b->h_gkeys, (size_t)n * 4, hipMemcpyHostToDevice, stream));
            a.keys = b->d_gkeys;
        }
        a.out_fid = b->d_gfid; a.out_grp = b->d_ggrp; a.out_sub = b->d_gsub; a.cap = total;
        HIP_OK(hipEventRecord(b->gev[2], stream));
        if (total) HIP_OK(launch_shared_pick(a, stream));
        HIP_OK(hipEventRecord(b->gev[3], stream));
    }
    out->n_topics = n;
    out->n_deliveries = total;
    if (o->flags & TM_SHARED_DEVICE) {
        HIP_OK(hipStreamSynchronize(stream));
    } else {
        if ((rc = host_reserve(b->h_grow, b->ch_grow, nn + 1))) return rc;
        HIP_OK(hipMemcpyAsync(b->h_grow, b->d_grow, ((size_t)n + 1) * 4, hipMemcpyDeviceToHost, stream));
        if (!counts_only) {
            if ((rc = host_reserve(b->h_gfid, b->ch_gfid, std::max<uint64_t>(total, 1)))) return rc;
            if ((rc = host_reserve(b->h_ggrp, b->ch_ggrp, std::max<uint64_t>(total, 1)))) return rc;
            if ((rc = host_reserve(b->h_gsub, b->ch_gsub, std::max<uint64_t>(total, 1)))) return rc;
            if (total) {
                HIP_OK(hipMemcpyAsync(b->h_gfid, b->d_gfid, total * 4, hipMemcpyDeviceToHost, stream));
                HIP_OK(hipMemcpyAsync(b->h_ggrp, b->d_ggrp, total * 4, hipMemcpyDeviceToHost, stream));
                HIP_OK(hipMemcpyAsync(b->h_gsub, b->d_gsub, total * 4, hipMemcpyDeviceToHost, stream));
            }
        }
        HIP_OK(hipStreamSynchronize(stream));
        if (b->h_grow[n] != total) {
            snprintf(last_error(), 512, "inconsistent shared delivery CSR: %u vs %llu", b->h_grow[n],
                     (unsigned long long)total);
            return TM_EIO;
        }
    }
    HIP_OK(hipEventElapsedTime(&ms, b->gev[0], b->gev[1]));
    if (!counts_only) HIP_OK(hipEventElapsedTime(&ms2, b->gev[2], b->gev[3]));
    out->kernel_ms = ms + ms2;
    const bool dev = o->flags & TM_SHARED_DEVICE;
    out->row_offsets = dev ? b->d_grow : b->h_grow;
    out->filter_ids = counts_only ? nullptr : dev ? b->d_gfid : b->h_gfid;
    out->groups = counts_only ? nullptr : dev ? b->d_ggrp : b->h_ggrp;
    out->subscribers = counts_only ? nullptr : dev ? b->d_gsub : b->h_gsub;
    return TM_OK;
}

// ---- C ABI

int tm_shared_subscribe(tm_engine* e, const uint8_t* topic, size_t len, uint32_t group_dest, uint32_t subscriber) {
    if (!e || (!topic && len)) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    try {
        return e->shared_subscribe(topic, len, group_dest, subscriber);
    } catch (...) {
        return TM_ENOMEM;
    }
}

int tm_shared_unsubscribe(tm_engine* e, const uint8_t* topic, size_t len, uint32_t group_dest, uint32_t subscriber) {
    if (!e || (!topic && len)) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    try {
        return e->shared_unsubscribe(topic, len, group_dest, subscriber);
    } catch (...) {
        return TM_ENOMEM;
    }
}

int tm_shared_member_down(tm_engine* e, uint32_t subscriber, uint64_t* n_removed) {
    if (!e) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    try {
        return e->shared_member_down(subscriber, n_removed);
    } catch (...) {
        return TM_ENOMEM;
    }
}

int tm_shared_members(tm_engine* e, const uint8_t* topic, size_t len, uint32_t group_dest, uint32_t* buf, uint32_t cap,
                      uint32_t* n) {
    if (!e || (!topic && len) || !n || (!buf && cap)) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    try {
        return e->shared_members(topic, len, group_dest, buf, cap, n);
    } catch (...) {
        return TM_ENOMEM;
    }
}

int tm_batch_dispatch_shared(tm_engine* e, tm_batch* b, const tm_shared_opts* opts, tm_shared_deliveries* out) {
    if (!e || !opts || !out) return TM_EINVAL;
    // the options are checked first, so a host-only engine reports them too
    if (opts->strategy > TM_SHARED_HASH) return einval("tm_batch_dispatch_shared: unknown strategy");
    if (opts->flags & ~(TM_SHARED_COUNT_ONLY | TM_SHARED_DEVICE)) return einval("tm_batch_dispatch_shared: unknown flag");
    if (opts->strategy == TM_SHARED_HASH && !opts->keys && !(opts->flags & TM_SHARED_COUNT_ONLY))
        return einval("tm_batch_dispatch_shared: TM_SHARED_HASH without keys");
    if (e->reps.empty()) return TM_ENODEV;   // host-only engine: no CPU fallback
    if (!b) return TM_EINVAL;
    if (!b->rep) return TM_ENODEV;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    int rc = e->use(b->rep);
    if (rc) return rc;
    try {
        return e->batch_dispatch_shared(b, opts, out);
    } catch (...) {
        return TM_ENOMEM;
    }
}
