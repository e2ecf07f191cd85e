// tm_shared.cpp -- shared subscriptions (emqx_shared_sub): the group membership
// bag, its device tables with the round-robin cursors, and the batched
// dispatch (tm_batch_dispatch_shared).  Table layout in tm_internal.hpp.
#include "tm_engine_impl.hpp"

static_assert(SH_RANDOM == TM_SHARED_RANDOM && SH_ROUND_ROBIN == TM_SHARED_ROUND_ROBIN && SH_HASH == TM_SHARED_HASH,
              "the kernels' strategy codes are the ABI's");

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
    max_sub = std::max(max_sub, sub);   // a member's deliveries are sorted with the others (armed inboxes)
    shared_dirty = true;
    return TM_OK;
}

int tm_engine::shared_subscribe_opts(const uint8_t* t, size_t len, uint32_t group, uint32_t sub, const tm_subopts& o) {
    tm_subopts* cur;
    const int frc = find_subopts(t, len, sub, &cur);
    if (frc == TM_OK) {
        // {SubPid, Topic} has options already, of either kind: the `true -> %% Existed`
        // branch (src/emqx_broker.erl:129-135) -- only the options merge
        const uint32_t mask = TM_SUBOPT_QOS | TM_SUBOPT_NL | TM_SUBOPT_RAP | TM_SUBOPT_RH | (o.subid ? TM_SUBOPT_SUBID : 0u);
        return set_subopts(t, len, sub, mask, o);
    }
    if (frc != TM_ENOENT) return frc;
    // the options first, taken back if the subscribe fails or throws
    shared_opts_of[sub].push_back(SharedOpt{std::string((const char*)t, len), group, o});
    int rc;
    try {
        rc = shared_subscribe(t, len, group, sub);
    } catch (...) {
        rc = TM_ENOMEM;
    }
    if (rc) {
        auto it = shared_opts_of.find(sub);
        it->second.pop_back();
        if (it->second.empty()) shared_opts_of.erase(it);
        return rc;
    }
    nl_entries += o.nl;
    subopts_dirty = true;
    return TM_OK;
}

void tm_engine::shared_opts_erase(const std::string& k, uint32_t group, uint32_t sub) {
    auto it = shared_opts_of.find(sub);
    if (it == shared_opts_of.end()) return;
    auto& v = it->second;
    for (auto e = v.begin(); e != v.end(); ++e)
        if (e->group == group && e->topic == k) {
            nl_entries -= e->o.nl;
            v.erase(e);
            subopts_dirty = true;
            break;
        }
    if (v.empty()) shared_opts_of.erase(it);
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
    shared_opts_erase(k, group, sub);   // ets:delete(?SUBOPTION, {SubPid, Topic}) (src/emqx_broker.erl:179-183)
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
    if ((rc = R.tab.d_goff.reserve(sn + 1))) return rc;
    if ((rc = R.tab.d_gcnt.reserve(std::max<size_t>(sn, 1)))) return rc;
    if ((rc = R.tab.d_gruns.reserve(std::max<size_t>(h_gruns.size(), 1)))) return rc;
    if ((rc = R.tab.d_gmem.reserve(std::max<size_t>(h_gmem.size(), 1)))) return rc;
    if ((rc = R.tab.d_gupd.reserve(std::max<size_t>(ns, 1)))) return rc;
    if (ns > R.tab.d_gslots.cap || !R.tab.d_gslots.p) {   // grown with the cursors kept; new slots start zeroed (epoch 0: never owned)
        const size_t old = R.tab.d_gslots.p ? R.tab.d_gslots.cap : 0;
        if ((rc = R.tab.d_gslots.reserve(std::max<size_t>(ns, 1), true, old))) return rc;
        HIP_OK(hipMemsetAsync(R.tab.d_gslots.p + old, 0, (R.tab.d_gslots.cap - old) * sizeof(SharedSlot), R.stream));
    }
    HIP_OK(hipMemcpyAsync(R.tab.d_goff.p, h_goff.data(), (sn + 1) * 4, hipMemcpyHostToDevice, R.stream));
    if (sn) HIP_OK(hipMemcpyAsync(R.tab.d_gcnt.p, h_gcnt.data(), sn, hipMemcpyHostToDevice, R.stream));
    if (!h_gruns.empty())
        HIP_OK(hipMemcpyAsync(R.tab.d_gruns.p, h_gruns.data(), h_gruns.size() * sizeof(uint4), hipMemcpyHostToDevice,
                              R.stream));
    if (!h_gmem.empty())
        HIP_OK(hipMemcpyAsync(R.tab.d_gmem.p, h_gmem.data(), h_gmem.size() * 4, hipMemcpyHostToDevice, R.stream));
    if (ns) {
        HIP_OK(hipMemcpyAsync(R.tab.d_gupd.p, h_gupd.data(), ns * sizeof(uint2), hipMemcpyHostToDevice, R.stream));
        HIP_OK(launch_shared_fold(R.tab.d_gslots.p, R.tab.d_gupd.p, (uint32_t)ns, R.stream));
    }
    HIP_OK(hipStreamSynchronize(R.stream));
    R.shared_gen = shared_gen;
    return TM_OK;
}

int tm_engine::batch_dispatch_shared(tm_batch* b, const tm_shared_opts* o, tm_shared_deliveries* out, bool entries) {
    if (!b->done) return einval("tm_batch_dispatch_shared: the batch has not been waited for");
    if (b->dedup) return einval("tm_batch_dispatch_shared: a TM_BATCH_DEDUP batch (the pick is per publish)");
    const bool counts_only = o->flags & TM_SHARED_COUNT_ONLY;
    const uint32_t n = b->n;
    Replica& R = *b->rep;
    const hipStream_t stream = R.stream;
    int rc;
    if ((rc = ensure_dense(b))) return rc;
    if ((rc = sync_shared(R))) return rc;
    const uint64_t m64 = b->total;   // match entries (< 2^32: u32 result CSR)
    if (m64 > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    const uint32_t m = (uint32_t)m64;
    tm_batch::Shared& sh = b->sh;
    if ((rc = sh.es.reserve(m, n))) return rc;
    if ((rc = sh.tot64.reserve(1))) return rc;
    for (Event& ev : sh.gev)
        if ((rc = ev.create())) return rc;
    SharedArgs a{};
    a.row_off = b->dcsr.d_rowoff.p; a.ids = b->dcsr.d_ids.p; a.n = n; a.m = m;
    a.gcnt = R.tab.d_gcnt.p; a.goff = R.tab.d_goff.p; a.runs = R.tab.d_gruns.p; a.mem = R.tab.d_gmem.p;
    a.nnodes = shared_nn; a.nruns = (uint32_t)h_gruns.size(); a.nmem = (uint32_t)h_gmem.size();
    a.nslots = (uint32_t)h_gupd.size(); a.slots = R.tab.d_gslots.p;
    a.ecount = sh.es.count.p; a.eoff = sh.es.eoff.p; a.bsums = sh.es.bsums.p; a.total = sh.es.total.d.p;
    a.total64 = sh.tot64.d.p; a.g_rowoff = sh.es.row.d.p;
    a.strategy = o->strategy; a.seed = o->seed;
    HIP_OK(hipEventRecord(sh.gev[0].e, stream));
    HIP_OK(hipMemsetAsync(sh.tot64.d.p, 0, 8, stream));
    HIP_OK(launch_shared_count(a, stream));
    HIP_OK(sh.es.scan(stream));
    HIP_OK(launch_shared_rows(a, stream));
    HIP_OK(hipEventRecord(sh.gev[1].e, stream));
    if ((rc = sh.tot64.fetch(1, stream))) return rc;
    HIP_OK(hipStreamSynchronize(stream));
    const uint64_t total = sh.tot64.h.p[0];
    if (total > 0xFFFFFFF0ull) return TM_EOVERFLOW;   // the u32 scan wrapped: nothing of it is used
    float ms = 0.f, ms2 = 0.f;
    if (!counts_only) {
        if ((rc = sh.fid.reserve(total))) return rc;
        if ((rc = sh.grp.reserve(total))) return rc;
        if ((rc = sh.sub.reserve(total))) return rc;
        if (o->strategy == TM_SHARED_HASH && n) {
            if ((rc = sh.keys.stage(o->keys, n, stream))) return rc;
            a.keys = sh.keys.d.p;
        }
        a.out_fid = sh.fid.d.p; a.out_grp = sh.grp.d.p; a.out_sub = sh.sub.d.p; a.cap = total;
        if (entries) {
            if ((rc = sh.d_gent.reserve(std::max<uint64_t>(total, 1)))) return rc;
            a.out_ent = sh.d_gent.p;
            // a slot the pick leaves unwritten reads as a pick without a member: the merge counts it
            if (total) HIP_OK(hipMemsetAsync(sh.sub.d.p, 0xFF, total * 4, stream));
        }
        HIP_OK(hipEventRecord(sh.gev[2].e, stream));
        if (total) HIP_OK(launch_shared_pick(a, stream));
        HIP_OK(hipEventRecord(sh.gev[3].e, stream));
    }
    const bool device = o->flags & TM_SHARED_DEVICE;
    if (!device) {
        if ((rc = sh.es.row.fetch((size_t)n + 1, stream))) return rc;
        if (!counts_only) {
            if ((rc = sh.fid.fetch(total, stream))) return rc;
            if ((rc = sh.grp.fetch(total, stream))) return rc;
            if ((rc = sh.sub.fetch(total, stream))) return rc;
        }
    }
    HIP_OK(hipStreamSynchronize(stream));
    if (!device && sh.es.row.h.p[n] != total) {
        snprintf(last_error(), 512, "inconsistent shared delivery CSR: %u vs %llu", sh.es.row.h.p[n],
                 (unsigned long long)total);
        return TM_EIO;
    }
    HIP_OK(hipEventElapsedTime(&ms, sh.gev[0].e, sh.gev[1].e));
    if (!counts_only) HIP_OK(hipEventElapsedTime(&ms2, sh.gev[2].e, sh.gev[3].e));
    out->n_topics = n;
    out->n_deliveries = total;
    out->kernel_ms = ms + ms2;
    out->row_offsets = sh.es.row.view(device);
    out->filter_ids = counts_only ? nullptr : sh.fid.view(device);
    out->groups = counts_only ? nullptr : sh.grp.view(device);
    out->subscribers = counts_only ? nullptr : sh.sub.view(device);
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

int tm_engine::batch_inbox_groups(tm_batch* b, uint32_t flags, const uint32_t** groups) {
    tm_batch::Inbox& ib = b->inbox;
    if (!b->shmode.armed || !ib.merged)
        return einval("tm_batch_inbox_groups: the batch is not armed, or no inboxes / deliver / window call ran armed");
    const bool device = flags & TM_INBOX_DEVICE;
    if (!device && !ib.grp_host) {
        const hipStream_t stream = b->rep->stream;
        if (int rc = ib.groups->fetch(ib.n_groups, stream)) return rc;
        HIP_OK(hipStreamSynchronize(stream));
        ib.grp_host = true;
    }
    *groups = ib.groups->view(device);
    return TM_OK;
}

int tm_batch_shared_mode(tm_engine* e, tm_batch* b, const tm_shared_opts* opts) {
    if (!e) return TM_EINVAL;
    // the options are checked first, so a host-only engine reports them too
    if (opts) {
        if (opts->strategy > TM_SHARED_HASH) return einval("tm_batch_shared_mode: unknown strategy");
        if (opts->flags & ~(TM_SHARED_COUNT_ONLY | TM_SHARED_DEVICE)) return einval("tm_batch_shared_mode: unknown flag");
        if (opts->flags)
            return einval("tm_batch_shared_mode: TM_SHARED_COUNT_ONLY / TM_SHARED_DEVICE have no meaning here");
        if (opts->strategy == TM_SHARED_HASH && !opts->keys) return einval("tm_batch_shared_mode: TM_SHARED_HASH without keys");
    }
    if (e->reps.empty()) return TM_ENODEV;   // host-only engine: no CPU fallback
    if (!b) return TM_EINVAL;
    if (!b->rep) return TM_ENODEV;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    if (!opts) {   // disarm: the batch behaves as before
        b->shmode.armed = false;
        b->shmode.keys.clear();
        return TM_OK;
    }
    if (b->dedup) return einval("tm_batch_shared_mode: a TM_BATCH_DEDUP batch (the pick is per publish)");
    try {
        if (opts->strategy == TM_SHARED_HASH) b->shmode.keys.assign(opts->keys, opts->keys + b->n);
        else b->shmode.keys.clear();
    } catch (...) {
        return TM_ENOMEM;
    }
    b->shmode.strategy = opts->strategy;
    b->shmode.seed = opts->seed;
    b->shmode.armed = true;
    return TM_OK;
}

int tm_batch_inbox_groups(tm_engine* e, tm_batch* b, uint32_t flags, const uint32_t** groups) {
    if (!e) return TM_EINVAL;
    if (!groups) return einval("tm_batch_inbox_groups: groups is NULL");
    if (flags & ~TM_INBOX_DEVICE) return einval("tm_batch_inbox_groups: unknown flag");
    if (e->reps.empty()) return TM_ENODEV;   // host-only engine: no CPU fallback
    if (!b) return TM_EINVAL;
    if (!b->rep) return TM_ENODEV;
    return on_batch(e, b, [&] { return e->batch_inbox_groups(b, flags, groups); });
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
    return on_batch(e, b, [&] { return e->batch_dispatch_shared(b, opts, out); });
}
