// tm_fanout.cpp -- routes (emqx_router), subscriptions and the fan-out dispatch
// (emqx_broker:publish -> subscribers), rule predicates.
#include "tm_engine_impl.hpp"

#include <memory>

int tm_engine::route_add(const uint8_t* t, size_t len, uint32_t dest) {
    uint32_t n = node_of(t, len);
    if (n == NONE || n >= n_nroutes.size() || n_nroutes[n] == 0) {
        int rc = trie_insert(t, len);     // first route: emqx_trie:insert/1 (idempotent)
        if (rc) return rc;
        n = node_of(t, len);
        if (n == NONE) return TM_EIO;
    }
    if (n_dests.size() < nd.size()) {
        n_dests.resize(nd.size());
        n_nroutes.resize(nd.size(), 0);
    }
    auto& v = n_dests[n];
    bool found = false;
    for (auto& e : v)
        if (e.first == dest) { ++e.second; found = true; break; }
    if (!found) {
        v.emplace_back(dest, 1u);
        ++route_entries;
        routes_dirty = true;
    }
    ++n_nroutes[n];
    ++version;
    return TM_OK;
}

int tm_engine::route_delete(const uint8_t* t, size_t len, uint32_t dest) {
    const uint32_t n = node_of(t, len);
    if (n == NONE || n >= n_dests.size()) return TM_ENOENT;
    auto& v = n_dests[n];
    size_t k = 0;
    while (k < v.size() && v[k].first != dest) ++k;
    if (k == v.size()) return TM_ENOENT;
    if (--v[k].second == 0) {
        v.erase(v.begin() + (long)k);
        --route_entries;
        routes_dirty = true;
    }
    --n_nroutes[n];
    ++version;
    if (n_nroutes[n] == 0) return trie_delete(t, len);   // last route: emqx_trie:delete/1
    return TM_OK;
}

int tm_engine::sync_routes(Replica& R) {
    if (routes_dirty || h_roff.size() < nd.size() + 1) {
        const size_t nn = nd.size();
        h_roff.assign(nn + 1, 0);
        h_rdest.clear();
        h_rdest.reserve(route_entries);
        for (size_t i = 0; i < nn; ++i) {
            h_roff[i] = (uint32_t)h_rdest.size();
            if (i < n_dests.size())
                for (const auto& e : n_dests[i]) h_rdest.push_back(e.first);
        }
        h_roff[nn] = (uint32_t)h_rdest.size();
        routes_dirty = false;
        ++routes_gen;
    }
    if (R.routes_gen == routes_gen) return TM_OK;
    const size_t nn = h_roff.size() - 1;
    int rc;
    if ((rc = R.tab.d_roff.reserve(nn + 1))) return rc;
    if ((rc = R.tab.d_rdest.reserve(std::max<size_t>(h_rdest.size(), 1)))) return rc;
    HIP_OK(hipMemcpyAsync(R.tab.d_roff.p, h_roff.data(), (nn + 1) * 4, hipMemcpyHostToDevice, R.stream));
    if (!h_rdest.empty())
        HIP_OK(hipMemcpyAsync(R.tab.d_rdest.p, h_rdest.data(), h_rdest.size() * 4, hipMemcpyHostToDevice, R.stream));
    HIP_OK(hipStreamSynchronize(R.stream));
    R.routes_gen = routes_gen;
    return TM_OK;
}

int tm_engine::batch_routes(tm_batch* b, tm_routes* out) {
    if (!b->done) return TM_EINVAL;
    Replica& R = *b->rep;
    const hipStream_t stream = R.stream;
    int rc;
    if ((rc = ensure_dense(b))) return rc;
    if ((rc = sync_routes(R))) return rc;
    const uint32_t n = b->n;
    const uint64_t m64 = b->total;   // match entries (< 2^32: u32 result CSR)
    if (m64 > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    const uint32_t m = (uint32_t)m64;
    tm_batch::Routes& rt = b->rt;
    if ((rc = rt.es.reserve(m, n))) return rc;
    RouteArgs r{};
    r.row_off = b->dcsr.d_rowoff.p; r.ids = b->dcsr.d_ids.p; r.n = n; r.m = m;
    r.roff = R.tab.d_roff.p; r.rdest = R.tab.d_rdest.p; r.nnodes = (uint32_t)(h_roff.size() - 1);
    r.ecount = rt.es.count.p; r.eoff = rt.es.eoff.p; r.bsums = rt.es.bsums.p; r.total = rt.es.total.d.p;
    r.r_rowoff = rt.es.row.d.p;
    HIP_OK(launch_route_count(r, stream));
    HIP_OK(rt.es.scan(stream));
    HIP_OK(launch_route_rows(r, stream));
    if ((rc = rt.es.total.fetch(1, stream))) return rc;
    HIP_OK(hipStreamSynchronize(stream));
    const uint64_t total = rt.es.total.h.p[0];
    if ((rc = rt.fid.reserve(total))) return rc;
    if ((rc = rt.dest.reserve(total))) return rc;
    r.out_fid = rt.fid.d.p; r.out_dest = rt.dest.d.p; r.cap = total;
    HIP_OK(launch_route_fill(r, stream));
    if ((rc = rt.es.row.fetch((size_t)n + 1, stream))) return rc;
    if ((rc = rt.fid.fetch(total, stream))) return rc;
    if ((rc = rt.dest.fetch(total, stream))) return rc;
    HIP_OK(hipStreamSynchronize(stream));
    if (rt.es.row.h.p[n] != total) {
        snprintf(last_error(), 512, "inconsistent route CSR: %u vs %llu", rt.es.row.h.p[n], (unsigned long long)total);
        return TM_EIO;
    }
    out->n_topics = n;
    out->n_routes = total;
    out->row_offsets = rt.es.row.h.p;
    out->filter_ids = rt.fid.h.p;
    out->dests = rt.dest.h.p;
    return TM_OK;
}

int tm_engine::subscribe(const uint8_t* t, size_t len, uint32_t sub, uint32_t node_dest) {
    return subscribe_opts(t, len, sub, node_dest, tm_subopts{});   // ?DEFAULT_SUBOPTS (include/emqx_mqtt.hrl:207-211)
}

int tm_engine::find_subopts(const uint8_t* t, size_t len, uint32_t sub, tm_subopts** out) {
    *out = nullptr;
    const std::string k((const char*)t, len);
    // an entry a shared subscribe stored (tm_shared_subscribe_opts)
    auto shi = shared_opts_of.find(sub);
    if (shi != shared_opts_of.end())
        for (auto& e : shi->second)
            if (e.topic == k) {
                *out = &e.o;
                return TM_OK;
            }
    auto it = topics_of.find(sub);
    if (it == topics_of.end()) return TM_ENOENT;
    auto ti = std::find(it->second.begin(), it->second.end(), k);
    if (ti == it->second.end()) return TM_ENOENT;
    auto oit = opts_of.find(sub);
    if (oit == opts_of.end() || oit->second.size() != it->second.size()) {
        snprintf(last_error(), 512, "subscriber %u: %zu topics, %zu option entries", sub, it->second.size(),
                 oit == opts_of.end() ? (size_t)0 : oit->second.size());
        return TM_EIO;
    }
    *out = &oit->second[(size_t)(ti - it->second.begin())];
    return TM_OK;
}

int tm_engine::set_subopts(const uint8_t* t, size_t len, uint32_t sub, uint32_t mask, const tm_subopts& o) {
    tm_subopts* cur;
    if (int rc = find_subopts(t, len, sub, &cur)) return rc;   // TM_ENOENT: set_subopts/2's `false` (:392)
    if (mask & TM_SUBOPT_QOS) cur->qos = o.qos;
    if (mask & TM_SUBOPT_NL) {
        nl_entries += o.nl;
        nl_entries -= cur->nl;
        cur->nl = o.nl;
    }
    if (mask & TM_SUBOPT_RAP) cur->rap = o.rap;
    if (mask & TM_SUBOPT_RH) cur->rh = o.rh;
    if (mask & TM_SUBOPT_SUBID) cur->subid = o.subid;
    subopts_dirty = true;
    return TM_OK;
}

int tm_engine::subscribe_opts(const uint8_t* t, size_t len, uint32_t sub, uint32_t node_dest, const tm_subopts& o) {
    std::string k((const char*)t, len);
    auto it = topics_of.find(sub);
    bool existed = it != topics_of.end() && std::find(it->second.begin(), it->second.end(), k) != it->second.end();
    if (!existed) {   // options a shared subscribe stored under {SubPid, Topic}: Existed as well
        auto shi = shared_opts_of.find(sub);
        if (shi != shared_opts_of.end())
            for (const auto& e : shi->second) existed = existed || e.topic == k;
    }
    if (existed) {
        // subscribed already: only the subopts change (:127-139) -- maps:merge(Old, New),
        // where New holds the four flags and a subid only when one was given (:139-142)
        const uint32_t mask = TM_SUBOPT_QOS | TM_SUBOPT_NL | TM_SUBOPT_RAP | TM_SUBOPT_RH | (o.subid ? TM_SUBOPT_SUBID : 0u);
        return set_subopts(t, len, sub, mask, o);
    }
    auto sit = subs_of.find(k);
    if (sit == subs_of.end()) {
        int rc = route_add(t, len, node_dest);
        if (rc) return rc;
        sit = subs_of.emplace(k, std::vector<uint32_t>()).first;
    }
    // the options first, and taken back if the bag's insert throws: opts_of[sub]
    // and topics_of[sub] stay index for index
    auto& os = opts_of[sub];
    os.push_back(o);
    try {
        auto& ts = topics_of[sub];
        ts.reserve(ts.size() + 1);
        sit->second.push_back(sub);
        ts.push_back(std::move(k));   // within the reserved capacity: does not throw
    } catch (...) {
        os.pop_back();
        if (os.empty()) opts_of.erase(sub);
        auto ti = topics_of.find(sub);
        if (ti != topics_of.end() && ti->second.empty()) topics_of.erase(ti);
        throw;
    }
    nl_entries += o.nl;
    max_sub = std::max(max_sub, sub);
    ++sub_entries;
    subs_dirty = true;
    subopts_dirty = true;
    return TM_OK;
}

int tm_engine::unsubscribe(const uint8_t* t, size_t len, uint32_t sub, uint32_t node_dest) {
    std::string k((const char*)t, len);
    auto it = topics_of.find(sub);
    if (it == topics_of.end()) return TM_ENOENT;
    auto& ts = it->second;
    auto ti = std::find(ts.begin(), ts.end(), k);
    if (ti == ts.end()) return TM_ENOENT;   // unsubscribe/1's `[] -> ok` (:170-177)
    {   // ets:delete(?SUBOPTION, {SubPid, Topic}) (:179-181)
        auto oit = opts_of.find(sub);
        if (oit == opts_of.end() || oit->second.size() != ts.size()) return TM_EIO;
        auto oi = oit->second.begin() + (ti - ts.begin());
        nl_entries -= oi->nl;
        oit->second.erase(oi);
        if (oit->second.empty()) opts_of.erase(oit);
        subopts_dirty = true;
    }
    ts.erase(ti);
    if (ts.empty()) topics_of.erase(it);
    auto sit = subs_of.find(k);
    if (sit == subs_of.end()) return TM_EIO;
    auto& v = sit->second;
    auto vi = std::find(v.begin(), v.end(), sub);
    if (vi == v.end()) return TM_EIO;
    v.erase(vi);
    --sub_entries;
    subs_dirty = true;
    if (v.empty()) {
        subs_of.erase(sit);
        int rc = route_delete(t, len, node_dest);
        if (rc && rc != TM_ENOENT) return rc;
    }
    return TM_OK;
}

int tm_engine::subscriber_down(uint32_t sub, uint32_t node_dest, uint64_t* n_removed) {
    uint64_t n = 0;
    auto it = topics_of.find(sub);
    if (it != topics_of.end()) {
        const std::vector<std::string> ts = it->second;
        for (const auto& k : ts) {
            int rc = unsubscribe((const uint8_t*)k.data(), k.size(), sub, node_dest);
            if (rc) return rc;
            ++n;
        }
    }
    if (n_removed) *n_removed = n;
    return TM_OK;
}

int tm_engine::sync_subs(Replica& R) {
    const size_t nn = nd.size();
    if (subs_dirty || subs_version != version || subs_nn != nn || h_soff.empty()) {
        h_soff.assign(nn + 1, 0);
        std::vector<std::pair<uint32_t, const std::vector<uint32_t>*>> runs;
        runs.reserve(subs_of.size());
        for (const auto& kv : subs_of) {
            const uint32_t n = node_of((const uint8_t*)kv.first.data(), kv.first.size());
            if (n == NONE || n >= nn) continue;   // not in the trie: no route, no dispatch
            runs.emplace_back(n, &kv.second);
            h_soff[n + 1] += kv.second.size();
        }
        for (size_t i = 0; i < nn; ++i) h_soff[i + 1] += h_soff[i];
        h_subs.resize(h_soff[nn]);
        for (const auto& r : runs) std::copy(r.second->begin(), r.second->end(), h_subs.begin() + (long)h_soff[r.first]);
        h_scnt.resize(std::max<size_t>(nn, 1));
        for (size_t i = 0; i < nn; ++i) h_scnt[i] = (uint8_t)std::min<uint64_t>(h_soff[i + 1] - h_soff[i], 255);
        h_sone.assign(std::max<size_t>(nn, 1), NONE);
        for (size_t i = 0; i < nn; ++i)
            if (h_soff[i + 1] - h_soff[i] == 1) h_sone[i] = h_subs[h_soff[i]];
        subs_dirty = false;
        subs_version = version;
        subs_nn = (uint32_t)nn;
        ++subs_gen;
    }
    if (R.subs_gen == subs_gen) return TM_OK;
    const size_t sn = subs_nn;
    int rc;
    if ((rc = R.tab.d_soff.reserve(sn + 1))) return rc;
    if ((rc = R.tab.d_scnt.reserve(std::max<size_t>(sn, 1)))) return rc;
    if ((rc = R.tab.d_sone.reserve(std::max<size_t>(sn, 1)))) return rc;
    if ((rc = R.tab.d_subs.reserve(std::max<size_t>(h_subs.size(), 1)))) return rc;
    HIP_OK(hipMemcpyAsync(R.tab.d_soff.p, h_soff.data(), (sn + 1) * 8, hipMemcpyHostToDevice, R.stream));
    if (sn) HIP_OK(hipMemcpyAsync(R.tab.d_scnt.p, h_scnt.data(), sn, hipMemcpyHostToDevice, R.stream));
    if (sn) HIP_OK(hipMemcpyAsync(R.tab.d_sone.p, h_sone.data(), sn * 4, hipMemcpyHostToDevice, R.stream));
    if (!h_subs.empty())
        HIP_OK(hipMemcpyAsync(R.tab.d_subs.p, h_subs.data(), h_subs.size() * 4, hipMemcpyHostToDevice, R.stream));
    HIP_OK(hipStreamSynchronize(R.stream));
    R.subs_gen = subs_gen;
    return TM_OK;
}

int tm_engine::batch_dispatch(tm_batch* b, uint32_t flags, tm_deliveries* out, bool entries) {
    if (!b->done) return TM_EINVAL;
    const bool rows = flags & TM_DISPATCH_ROWS;
    if (rows && ((flags & TM_DISPATCH_MATCH_OFFSETS) || !b->csr)) return TM_EINVAL;
    if (rows) flags |= TM_DISPATCH_DEVICE;
    Replica& R = *b->rep;
    const hipStream_t stream = R.stream;
    int rc;
    if (!rows && (rc = ensure_dense(b))) return rc;
    if ((rc = sync_subs(R))) return rc;
    const uint32_t n = b->n;
    tm_batch::Fanout& fan = b->fan;
    FanArgs fa{};
    uint64_t nm = b->total;
    if (rows) {   // the walk's staging regions as one virtual entry space (FanArgs)
        const uint64_t cap = std::min<uint64_t>(b->walk.d_sfids.cap, MAX_RESULT);
        fa.nreg = b->one_region ? 1u : TICKET_GROUPS;
        fa.rcap = region_cap(cap, b->one_region);
        // [vb: TICKET_GROUPS + 1 | rtop: TICKET_GROUPS] -> HBM
        constexpr size_t FM = 2 * TICKET_GROUPS + 1;
        uint64_t fm[FM] = {};
        uint64_t *vb = fm, *rtop = fm + TICKET_GROUPS + 1;
        uint64_t v = 0, staged = 0;
        for (uint32_t g = 0; g < fa.nreg; ++g) {
            vb[g] = v;
            rtop[g] = xg_top_read(b->walk.h_ctrl, g);
            staged += rtop[g];
            v += (rtop[g] + 15) & ~15ull;
        }
        for (uint32_t g = fa.nreg; g <= TICKET_GROUPS; ++g) vb[g] = v;
        if ((rc = fan.meta.stage(fm, FM, stream))) return rc;
        fa.vb = fan.meta.d.p;
        fa.rtop = fan.meta.d.p + TICKET_GROUPS + 1;
        if (staged != b->total) {
            snprintf(last_error(), 512, "staging holds %llu entries, the walk matched %llu",
                     (unsigned long long)staged, (unsigned long long)b->total);
            return TM_EIO;
        }
        nm = v;
        if ((rc = fan.d_dcount.reserve(std::max<size_t>(n, 1)))) return rc;
        fa.rcount = b->walk.d_count;
        fa.rsrc = b->walk.d_src;
        fa.dcount = fan.d_dcount.p;
    }
    const uint32_t nb = (uint32_t)((nm + 1 + fan_scan_tile() - 1) / fan_scan_tile());
    if ((rc = fan.moff.reserve(nm + 1))) return rc;
    if ((rc = fan.d_fbsums.reserve(nb))) return rc;
    if ((rc = fan.d_moff32.reserve(nm + 1))) return rc;
    if ((rc = fan.d_fbig.reserve(nb))) return rc;
    if ((rc = fan.total.reserve(1))) return rc;
    if ((rc = fan.row.reserve((size_t)n + 1))) return rc;
    const bool counts_only = flags & TM_DISPATCH_COUNT_ONLY;
    if (!fan.fev0.e) {
        if ((rc = fan.fev0.create())) return rc;
        if ((rc = fan.fev1.create())) return rc;
    }
    fa.row_off = b->dcsr.d_rowoff.p; fa.ids = rows ? b->walk.d_sfids.p : b->dcsr.d_ids.p; fa.n = n; fa.n_matches = nm;
    fa.soff = R.tab.d_soff.p; fa.scnt = R.tab.d_scnt.p; fa.sone = R.tab.d_sone.p; fa.subs = R.tab.d_subs.p;
    fa.nnodes = subs_nn;
    fa.moff = fan.moff.d.p; fa.moff32 = fan.d_moff32.p; fa.bbig = fan.d_fbig.p; fa.bsums = fan.d_fbsums.p;
    fa.big_limit = fan_big_limit; fa.d_total = fan.total.d.p; fa.drow = fan.row.d.p;
    HIP_OK(launch_fan_scan(fa, stream));
    if ((rc = fan.total.fetch(1, stream))) return rc;
    HIP_OK(hipStreamSynchronize(stream));
    const uint64_t total = fan.total.h.p[0];
    float fill_ms = 0.f;
    if (!counts_only) {
        if ((rc = fan.out.reserve(total))) return rc;
        if ((rc = fan.d_ftile.reserve((size_t)(total / fan_fill_tile()) + 2))) return rc;
        fa.out = fan.out.d.p; fa.total = total; fa.tile_j = fan.d_ftile.p;
        if (entries) {
            if (total > MAX_RESULT) return TM_EOVERFLOW;   // the sort's payload and the inbox offsets are u32
            if ((rc = b->inbox.d_val0.reserve(std::max<uint64_t>(total, 1)))) return rc;
            fa.out_j = b->inbox.d_val0.p;
        }
        HIP_OK(hipEventRecord(fan.fev0.e, stream));
        HIP_OK(launch_fan_fill(fa, stream));
        HIP_OK(hipEventRecord(fan.fev1.e, stream));
    }
    const bool want_moff = flags & TM_DISPATCH_MATCH_OFFSETS;
    if (want_moff) HIP_OK(launch_fan_globalize(fa, stream));   // moff is block-relative until now
    const bool device = flags & TM_DISPATCH_DEVICE;
    if (!device) {
        if ((rc = fan.row.fetch((size_t)n + 1, stream))) return rc;
        if (want_moff && (rc = fan.moff.fetch(nm + 1, stream))) return rc;
        if (!counts_only && (rc = fan.out.fetch(total, stream))) return rc;
    }
    HIP_OK(hipStreamSynchronize(stream));
    if (!counts_only) HIP_OK(hipEventElapsedTime(&fill_ms, fan.fev0.e, fan.fev1.e));
    if (!device && fan.row.h.p[n] != total) {
        snprintf(last_error(), 512, "inconsistent delivery CSR: %llu vs %llu", (unsigned long long)fan.row.h.p[n],
                 (unsigned long long)total);
        return TM_EIO;
    }
    out->n_topics = n;
    out->n_matches = b->total;
    out->n_deliveries = total;
    out->row_offsets = fan.row.view(device);
    out->match_offsets = want_moff ? fan.moff.view(device) : nullptr;
    out->subscribers = counts_only ? nullptr : fan.out.view(device);
    out->fill_ms = fill_ms;
    out->row_counts = rows ? fan.d_dcount.p : nullptr;
    return TM_OK;
}

int tm_engine::batch_inboxes(tm_batch* b, uint32_t flags, tm_inboxes* out) {
    if (!b->done) return einval("tm_batch_inboxes: the batch has not been waited for");
    if (b->dedup) return einval("tm_batch_inboxes: a TM_BATCH_DEDUP batch (an inbox entry names a publish)");
    if (b->total > MAX_RESULT) return TM_EOVERFLOW;
    // armed (tm_batch_shared_mode): the sort runs over L', the fan-out's
    // deliveries merged with one pick per (entry, group)
    const bool armed = b->shmode.armed;
    if (armed && b->shmode.strategy == TM_SHARED_HASH && b->shmode.keys.size() != b->n)
        return einval("tm_batch_inboxes: the batch was re-prepared since tm_batch_shared_mode copied its keys");
    tm_deliveries dl{};
    int rc;
    // returns with the stream idle
    if ((rc = batch_dispatch(b, TM_DISPATCH_DEVICE | (armed ? TM_DISPATCH_MATCH_OFFSETS : 0u), &dl, true))) return rc;
    Replica& R = *b->rep;
    const hipStream_t stream = R.stream;
    tm_batch::Inbox& ib = b->inbox;
    ib.merged = false;
    ib.grp_host = false;
    ib.groups = nullptr;
    ib.n_groups = 0;
    ib.key0 = b->fan.out.d.p;
    const uint32_t n = b->n, m = (uint32_t)b->total;
    const uint32_t D0 = (uint32_t)dl.n_deliveries;   // <= MAX_RESULT (batch_dispatch checked)
    uint32_t DS = 0;                                  // shared deliveries
    if (armed) {
        const tm_shared_opts so{b->shmode.strategy, TM_SHARED_DEVICE, b->shmode.keys.data(), b->shmode.seed};
        tm_shared_deliveries sd{};
        if ((rc = batch_dispatch_shared(b, &so, &sd, true))) return rc;   // returns with the stream idle
        if ((uint64_t)D0 + sd.n_deliveries > MAX_RESULT) return TM_EOVERFLOW;
        DS = (uint32_t)sd.n_deliveries;
    }
    const uint32_t D = D0 + DS;
    const uint32_t ntiles = (uint32_t)(((uint64_t)D + INBOX_TILE - 1) / INBOX_TILE);
    const uint32_t bits = max_sub ? 32u - (uint32_t)__builtin_clz(max_sub) : 0u;
    const uint32_t passes = std::max(1u, (bits + 7) / 8);
    // a subscriber with a delivery has a subscription: R <= both
    const uint32_t rcap = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(D, topics_of.size() + (armed ? shared_topics_of.size() : 0)));
    const size_t dd = std::max<size_t>(D, 1), nh = (size_t)256 * ntiles;
    if ((rc = ib.d_key1.reserve(dd))) return rc;
    if ((rc = ib.d_val1.reserve(dd))) return rc;
    if ((rc = ib.d_pubof.reserve(std::max<size_t>(m, 1)))) return rc;
    if ((rc = ib.d_hist.reserve(nh + 1))) return rc;
    if ((rc = ib.d_hbs.reserve((size_t)scan_block_count((uint32_t)nh) + 1))) return rc;
    if ((rc = ib.d_hcount.reserve((size_t)ntiles + 1))) return rc;
    if ((rc = ib.d_hcbs.reserve((size_t)scan_block_count(ntiles) + 1))) return rc;
    if ((rc = ib.d_R.reserve(1))) return rc;
    if ((rc = ib.h_R.reserve(2))) return rc;
    ib.h_R.p[1] = 0;
    if ((rc = ib.pub.reserve(D))) return rc;
    if ((rc = ib.fid.reserve(D))) return rc;
    if ((rc = ib.sub.reserve(rcap))) return rc;
    if ((rc = ib.off.reserve((size_t)rcap + 1))) return rc;
    if ((rc = ib.iev0.create())) return rc;
    if ((rc = ib.iev1.create())) return rc;
    InboxArgs a{};
    a.row_off = b->dcsr.d_rowoff.p; a.ids = b->dcsr.d_ids.p; a.n = n; a.m = m; a.D = D; a.ntiles = ntiles;
    a.passes = passes; a.pub_of = ib.d_pubof.p;
    a.key0 = b->fan.out.d.p; a.val0 = ib.d_val0.p; a.key1 = ib.d_key1.p; a.val1 = ib.d_val1.p;
    a.hist = ib.d_hist.p; a.hbs = ib.d_hbs.p; a.rcap = rcap; a.hcount = ib.d_hcount.p; a.hcbs = ib.d_hcbs.p;
    a.d_R = ib.d_R.p; a.publishes = ib.pub.d.p; a.filter_ids = ib.fid.d.p; a.subscribers = ib.sub.d.p;
    a.inbox_offsets = ib.off.d.p;
    MergeArgs ma{};
    if (armed) {
        if ((rc = ib.d_mkey.reserve(dd))) return rc;
        if ((rc = ib.d_mval.reserve(dd))) return rc;
        if ((rc = ib.d_mrec.reserve(dd))) return rc;
        if ((rc = ib.grp.reserve(D))) return rc;
        if ((rc = ib.d_merr.reserve(1))) return rc;
        ma.fsub = b->fan.out.d.p; ma.fent = ib.d_val0.p; ma.nd = D0;
        ma.gsub = b->sh.sub.d.p; ma.ggrp = b->sh.grp.d.p; ma.gent = b->sh.d_gent.p; ma.ns = DS;
        ma.m = m; ma.moff = b->fan.moff.d.p; ma.eoff = b->sh.es.eoff.p; ma.bsums = b->sh.es.bsums.p;
        ma.pub_of = ib.d_pubof.p; ma.ids = b->dcsr.d_ids.p;
        ma.cap = D; ma.key = ib.d_mkey.p; ma.val = ib.d_mval.p; ma.rec = ib.d_mrec.p;
        ma.err = ib.d_merr.p;
        a.key0 = ib.d_mkey.p; a.val0 = ib.d_mval.p;
        a.mrec = ib.d_mrec.p; a.groups = ib.grp.d.p;
        ib.key0 = ib.d_mkey.p;
        ib.merged = true;
        ib.groups = &ib.grp;
        ib.n_groups = D;
    }
    uint32_t nsub = 0;
    float ms = 0.f;
    if (D) {
        HIP_OK(hipEventRecord(ib.iev0.e, stream));
        HIP_OK(launch_inbox_pubof(a, stream));
        if (armed) {   // behind pubof: the merge stores every delivery's publish
            HIP_OK(hipMemsetAsync(ib.d_merr.p, 0, 4, stream));
            HIP_OK(launch_inbox_merge(ma, stream));
        }
        HIP_OK(launch_inbox_sort(a, stream));
        HIP_OK(launch_inbox_finish(a, stream));
        HIP_OK(hipEventRecord(ib.iev1.e, stream));
        HIP_OK(hipMemcpyAsync(ib.h_R.p, ib.d_R.p, 4, hipMemcpyDeviceToHost, stream));
        if (armed) HIP_OK(hipMemcpyAsync(ib.h_R.p + 1, ib.d_merr.p, 4, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        HIP_OK(hipEventElapsedTime(&ms, ib.iev0.e, ib.iev1.e));
        if (ib.h_R.p[1]) {   // a group route without a member cannot happen under the engine lock
            snprintf(last_error(), 512, "tm_batch_inboxes: %u of %u + %u deliveries without a member or out of place in the merge",
                     ib.h_R.p[1], D0, DS);
            return TM_EIO;
        }
        nsub = ib.h_R.p[0];
        if (nsub == 0 || nsub > rcap) {
            snprintf(last_error(), 512, "inconsistent inboxes: %u subscribers for %u deliveries (capacity %u)", nsub, D, rcap);
            return TM_EIO;
        }
    } else {
        HIP_OK(hipMemsetAsync(ib.off.d.p, 0, 4, stream));   // inbox_offsets = {0}
        HIP_OK(hipStreamSynchronize(stream));
    }
    out->n_topics = n;
    out->n_subscribers = nsub;
    out->n_deliveries = D;
    out->kernel_ms = ms;
    out->passes = D ? passes : 0;
    const bool device = flags & TM_INBOX_DEVICE;
    if (!device) {
        if ((rc = ib.off.fetch((size_t)nsub + 1, stream))) return rc;
        if ((rc = ib.sub.fetch(nsub, stream))) return rc;
        if ((rc = ib.pub.fetch(D, stream))) return rc;
        if ((rc = ib.fid.fetch(D, stream))) return rc;
        HIP_OK(hipStreamSynchronize(stream));
        if (ib.off.h.p[nsub] != D) {
            snprintf(last_error(), 512, "inconsistent inbox offsets: %u vs %u", ib.off.h.p[nsub], D);
            return TM_EIO;
        }
    }
    out->subscribers = ib.sub.view(device); out->inbox_offsets = ib.off.view(device);
    out->publishes = ib.pub.view(device); out->filter_ids = ib.fid.view(device);
    return TM_OK;
}

static_assert(DLV_UPGRADE_QOS == TM_DELIVER_UPGRADE_QOS && DLV_NL_ALL == TM_DELIVER_NL_ALL, "TM_DELIVER_* flags");
static_assert(MSG_RETAIN == TM_MSG_RETAIN && MSG_RETAINED == TM_MSG_RETAINED && MSG_NL == TM_MSG_NL, "TM_MSG_* bits");
static_assert(TM_SUBID_MAX >> (32 - SO_SUBID_SHIFT) == 0, "a subid fits the table's payload word");

int tm_engine::sync_subopts(Replica& R) {
    const size_t nn = nd.size();
    if (subopts_dirty || subopts_version != version || subopts_nn != nn || h_tstart.empty()) {
        h_tsub.clear();
        h_tsub.reserve(topics_of.size() + shared_opts_of.size());
        for (const auto& kv : topics_of) h_tsub.push_back(kv.first);
        for (const auto& kv : shared_opts_of)
            if (!topics_of.count(kv.first)) h_tsub.push_back(kv.first);
        std::sort(h_tsub.begin(), h_tsub.end());
        h_tstart.assign(h_tsub.size() + 1, 0);
        h_tnode.clear();
        h_tval.clear();
        h_tnode.reserve(sub_entries + shared_opts_of.size());
        h_tval.reserve(sub_entries + shared_opts_of.size());
        std::vector<std::pair<uint32_t, uint32_t>> row;
        static const std::vector<std::string> no_topics;
        static const std::vector<tm_subopts> no_opts;
        for (size_t s = 0; s < h_tsub.size(); ++s) {
            const auto tit = topics_of.find(h_tsub[s]);
            const auto oit = opts_of.find(h_tsub[s]);
            const auto& ts = tit == topics_of.end() ? no_topics : tit->second;
            const auto& os = oit == opts_of.end() ? no_opts : oit->second;
            if (os.size() != ts.size()) {
                snprintf(last_error(), 512, "subscriber %u: %zu topics, %zu option entries", h_tsub[s], ts.size(), os.size());
                return TM_EIO;
            }
            row.clear();
            auto add = [&](const std::string& t, const tm_subopts& o) {
                const uint32_t n = node_of((const uint8_t*)t.data(), t.size());
                if (n == NONE || n >= nn) return;   // not in the trie: no route, no dispatch (sync_subs)
                row.emplace_back(n, o.subid << SO_SUBID_SHIFT | (o.rap ? SO_RAP : 0u) | (o.nl ? SO_NL : 0u) | (o.qos & SO_QOS));
            };
            for (size_t i = 0; i < ts.size(); ++i) add(ts[i], os[i]);
            const auto shi = shared_opts_of.find(h_tsub[s]);
            if (shi != shared_opts_of.end())
                for (const auto& e : shi->second) add(e.topic, e.o);
            std::sort(row.begin(), row.end());
            h_tstart[s] = (uint32_t)h_tnode.size();
            for (const auto& e : row) {
                h_tnode.push_back(e.first);
                h_tval.push_back(e.second);
            }
        }
        h_tstart[h_tsub.size()] = (uint32_t)h_tnode.size();
        subopts_dirty = false;
        subopts_version = version;
        subopts_nn = (uint32_t)nn;
        ++subopts_gen;
    }
    if (R.subopts_gen == subopts_gen) return TM_OK;
    const size_t ns = h_tsub.size(), nt = h_tnode.size();
    int rc;
    if ((rc = R.tab.d_tsub.reserve(std::max<size_t>(ns, 1)))) return rc;
    if ((rc = R.tab.d_tstart.reserve(ns + 1))) return rc;
    if ((rc = R.tab.d_tnode.reserve(std::max<size_t>(nt, 1)))) return rc;
    if ((rc = R.tab.d_tval.reserve(std::max<size_t>(nt, 1)))) return rc;
    if (ns) HIP_OK(hipMemcpyAsync(R.tab.d_tsub.p, h_tsub.data(), ns * 4, hipMemcpyHostToDevice, R.stream));
    HIP_OK(hipMemcpyAsync(R.tab.d_tstart.p, h_tstart.data(), (ns + 1) * 4, hipMemcpyHostToDevice, R.stream));
    if (nt) {
        HIP_OK(hipMemcpyAsync(R.tab.d_tnode.p, h_tnode.data(), nt * 4, hipMemcpyHostToDevice, R.stream));
        HIP_OK(hipMemcpyAsync(R.tab.d_tval.p, h_tval.data(), nt * 4, hipMemcpyHostToDevice, R.stream));
    }
    HIP_OK(hipStreamSynchronize(R.stream));
    R.subopts_gen = subopts_gen;
    return TM_OK;
}

int tm_engine::batch_deliver(tm_batch* b, const tm_deliver_opts* o, tm_session_inboxes* out) {
    if (!b->done) return einval("tm_batch_deliver: the batch has not been waited for");
    if (b->dedup) return einval("tm_batch_deliver: a TM_BATCH_DEDUP batch (a delivery names a publish)");
    const uint32_t n = b->n;
    if (o->msg)
        for (uint32_t i = 0; i < n; ++i)
            if ((o->msg[i] & ~0xFu) || (o->msg[i] & 3u) == 3u)
                return einval("tm_batch_deliver: msg[%u] = 0x%02x (QoS 3 or bits above 3)", i, o->msg[i]);
    const bool device = o->flags & TM_DELIVER_DEVICE, want_subids = o->flags & TM_DELIVER_SUBIDS;
    // nothing can drop without a publisher or without a No-Local subscription
    const bool can_drop = o->from && nl_entries > 0;
    tm_inboxes ibx{};
    int rc;
    if ((rc = batch_inboxes(b, (device || can_drop) ? TM_INBOX_DEVICE : 0u, &ibx))) return rc;   // returns with the stream idle
    Replica& R = *b->rep;
    const hipStream_t stream = R.stream;
    tm_batch::Inbox& ib = b->inbox;
    tm_batch::Deliver& dv = b->dlv;
    const uint32_t D = (uint32_t)ibx.n_deliveries, nsub = ibx.n_subscribers;
    const size_t dd = std::max<size_t>(D, 1);
    *out = tm_session_inboxes{};
    out->n_topics = n;
    if ((rc = dv.msg.reserve(D))) return rc;
    if (want_subids && (rc = dv.subid.reserve(D))) return rc;
    if (!D) {   // no delivery: n_subscribers = 0, inbox_offsets = {0}
        if (device) {
            out->inbox_offsets = ib.off.d.p;
            out->subscribers = ib.sub.d.p; out->publishes = ib.pub.d.p; out->filter_ids = ib.fid.d.p;
        } else {   // nothing to copy: the pinned sides alone, the offset written here
            if ((rc = dv.off.fetch(0, stream))) return rc;
            if ((rc = dv.sub.fetch(0, stream))) return rc;
            if ((rc = dv.msg.fetch(0, stream))) return rc;
            if (want_subids && (rc = dv.subid.fetch(0, stream))) return rc;
            dv.off.h.p[0] = 0;
            out->inbox_offsets = dv.off.h.p;
            out->subscribers = out->publishes = out->filter_ids = dv.sub.h.p;
        }
        out->msg = dv.msg.view(device);
        out->subids = want_subids ? dv.subid.view(device) : nullptr;
        return TM_OK;
    }
    if ((rc = sync_subopts(R))) return rc;
    const uint32_t ntiles = (uint32_t)(((uint64_t)D + INBOX_TILE - 1) / INBOX_TILE);
    if ((rc = dv.d_rng.reserve(nsub))) return rc;
    if ((rc = dv.d_first.reserve(nsub))) return rc;
    if ((rc = dv.tot.reserve(4))) return rc;
    if ((rc = dv.dev0.create())) return rc;
    if ((rc = dv.dev1.create())) return rc;
    DeliverArgs a{};
    a.keys = ibx.passes & 1 ? ib.d_key1.p : ib.key0;   // where the sort left the pairs
    a.groups = ib.merged ? ib.grp.d.p : nullptr;
    a.publishes = ib.pub.d.p; a.filter_ids = ib.fid.d.p; a.subscribers = ib.sub.d.p;
    a.hcount = ib.d_hcount.p; a.hcbs = ib.d_hcbs.p;
    a.D = D; a.R = nsub; a.n = n; a.ntiles = ntiles;
    a.tsub = R.tab.d_tsub.p; a.tstart = R.tab.d_tstart.p; a.tnode = R.tab.d_tnode.p; a.tval = R.tab.d_tval.p;
    a.T = (uint32_t)h_tnode.size(); a.NS = (uint32_t)h_tsub.size();
    a.flags = o->flags;
    a.rng = dv.d_rng.p; a.first = dv.d_first.p;
    a.err = dv.tot.d.p + 2; a.d_tot = dv.tot.d.p;
    if (o->msg) {
        if ((rc = dv.msg_in.stage(o->msg, n, stream))) return rc;
        a.msg = dv.msg_in.d.p;
    }
    if (can_drop) {
        if ((rc = dv.from.stage(o->from, n, stream))) return rc;
        a.from = dv.from.d.p;
        if ((rc = dv.d_own.reserve(dd))) return rc;
        if ((rc = dv.d_emsg.reserve(dd))) return rc;
        if (want_subids && (rc = dv.d_esubid.reserve(dd))) return rc;
        if ((rc = dv.d_kcount.reserve((size_t)ntiles + 1))) return rc;
        if ((rc = dv.d_kbs.reserve((size_t)scan_block_count(ntiles) + 1))) return rc;
        if ((rc = dv.d_ncount.reserve((size_t)ntiles + 1))) return rc;
        if ((rc = dv.d_nbs.reserve((size_t)scan_block_count(ntiles) + 1))) return rc;
        if ((rc = dv.sub.reserve(nsub))) return rc;
        if ((rc = dv.off.reserve((size_t)nsub + 1))) return rc;
        if ((rc = dv.pub.reserve(D))) return rc;
        if ((rc = dv.fid.reserve(D))) return rc;
        if (ib.merged) {
            if ((rc = dv.grp.reserve(D))) return rc;
            a.o_grp = dv.grp.d.p;
        }
        a.own = dv.d_own.p; a.emsg = dv.d_emsg.p; a.esubid = want_subids ? dv.d_esubid.p : nullptr;
        a.kcount = dv.d_kcount.p; a.kbs = dv.d_kbs.p; a.ncount = dv.d_ncount.p; a.nbs = dv.d_nbs.p;
        a.o_sub = dv.sub.d.p; a.o_off = dv.off.d.p; a.o_pub = dv.pub.d.p; a.o_fid = dv.fid.d.p;
        a.o_msg = dv.msg.d.p; a.o_subid = want_subids ? dv.subid.d.p : nullptr;
    } else {   // the enriched bytes are the result; the other four arrays are the inboxes'
        a.emsg = dv.msg.d.p; a.esubid = want_subids ? dv.subid.d.p : nullptr;
    }
    HIP_OK(hipMemsetAsync(dv.tot.d.p, 0, 16, stream));
    HIP_OK(hipEventRecord(dv.dev0.e, stream));
    HIP_OK(launch_deliver_flags(a, can_drop, stream));
    if (can_drop) HIP_OK(launch_deliver_compact(a, stream));
    HIP_OK(hipEventRecord(dv.dev1.e, stream));
    if ((rc = dv.tot.fetch(4, stream))) return rc;
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipEventElapsedTime(&out->kernel_ms, dv.dev0.e, dv.dev1.e));
    const uint32_t* tot = dv.tot.h.p;   // [deliveries left, inboxes left, errors]
    if (tot[2]) {
        snprintf(last_error(), 512, "tm_batch_deliver: %u of %u deliveries without subscription options", tot[2], D);
        return TM_EIO;
    }
    const uint32_t left = can_drop ? tot[0] : D, rleft = can_drop ? tot[1] : nsub;
    if (left > D || rleft > nsub || (left == 0) != (rleft == 0)) {
        snprintf(last_error(), 512, "inconsistent session inboxes: %u of %u deliveries, %u of %u subscribers", left, D,
                 rleft, nsub);
        return TM_EIO;
    }
    out->n_subscribers = rleft;
    out->n_deliveries = left;
    out->n_dropped_no_local = D - left;
    if (ib.merged && can_drop) {   // tm_batch_inbox_groups: compacted alike
        ib.groups = &dv.grp;
        ib.n_groups = left;
        ib.grp_host = false;
    }
    if (!device) {
        if ((rc = dv.msg.fetch(left, stream))) return rc;
        if (want_subids && (rc = dv.subid.fetch(left, stream))) return rc;
        if (can_drop) {
            if ((rc = dv.off.fetch(rleft ? (size_t)rleft + 1 : 0, stream))) return rc;
            if ((rc = dv.sub.fetch(rleft, stream))) return rc;
            if ((rc = dv.pub.fetch(left, stream))) return rc;
            if ((rc = dv.fid.fetch(left, stream))) return rc;
        }
        HIP_OK(hipStreamSynchronize(stream));
        if (can_drop) {
            if (!rleft) dv.off.h.p[0] = 0;
            if (dv.off.h.p[rleft] != left) {
                snprintf(last_error(), 512, "inconsistent session inbox offsets: %u vs %u", dv.off.h.p[rleft], left);
                return TM_EIO;
            }
        }
    }
    if (can_drop) {
        out->subscribers = dv.sub.view(device); out->inbox_offsets = dv.off.view(device);
        out->publishes = dv.pub.view(device); out->filter_ids = dv.fid.view(device);
    } else {   // nothing dropped: the inboxes' own arrays
        out->subscribers = ibx.subscribers; out->inbox_offsets = ibx.inbox_offsets;
        out->publishes = ibx.publishes; out->filter_ids = ibx.filter_ids;
    }
    out->msg = dv.msg.view(device);
    out->subids = want_subids ? dv.subid.view(device) : nullptr;
    return TM_OK;
}

static_assert(WIN_DISCONNECTED == TM_SESS_DISCONNECTED && WIN_STORE_QOS0 == TM_SESS_STORE_QOS0 && WIN_HOST == TM_SESS_HOST,
              "TM_SESS_* flags");
static_assert(WIN_NDISP == TM_DISP_COUNT && TM_DISP_SEND0 == 0 && TM_DISP_SEND == 1 && TM_DISP_QUEUED == 2 &&
                  TM_DISP_DROP_QOS0 == 3 && TM_DISP_DROP_FULL == 4 && TM_DISP_HOST == 5,
              "TM_DISP_* as tm_window_classify stores them");
static_assert(sizeof(tm_session_state) == WIN_SESSION_WORDS * 4 && std::has_unique_object_representations_v<tm_session_state>,
              "tm_session_state is uploaded as six words");
static_assert(sizeof(tm_window_opts) == 40 && std::has_unique_object_representations_v<tm_window_opts>,
              "tm_window_opts has implicit padding");
static_assert(sizeof(tm_window_record) == sizeof(uint4) && std::has_unique_object_representations_v<tm_window_record>,
              "tm_window_record is the kernels' uint4");
static_assert(sizeof(tm_session_window) == sizeof(tm_session_inboxes) + 3 * sizeof(void*) + 8 * TM_DISP_COUNT + 8,
              "tm_session_window has implicit padding");

// ---- priority tables (tm_ptable_create, tm_batch_window_prio)
static_assert(PRIO_CLASSES == TM_PRIO_MAX_CLASSES && PRIO_NOCLASS == TM_PRIO_NOCLASS && PRIO_MAX_KEY == TM_MAX_TOPIC_LEN,
              "TM_PRIO_* as the kernels use them");
static_assert(sizeof(tm_session_prio) == PRIO_SESSION_WORDS * 4 && std::has_unique_object_representations_v<tm_session_prio>,
              "tm_session_prio is uploaded as ten words");
static_assert(sizeof(tm_window_prio_opts) == 32 && std::has_unique_object_representations_v<tm_window_prio_opts>,
              "tm_window_prio_opts has implicit padding");
static_assert(sizeof(tm_prio_record) == sizeof(uint2) && std::has_unique_object_representations_v<tm_prio_record>,
              "tm_prio_record is the kernels' uint2");
static_assert(sizeof(tm_window_prio) == 2 * sizeof(void*) + 8, "tm_window_prio has implicit padding");

// dd_hash (tm_kernels.hip) on the host, bit for bit: NH over the first 64
// bytes as little-endian words, the bytes past them chained 8 at a time, the
// length, the finaliser.
static uint64_t prio_hash(const uint8_t* p, uint32_t len) {
    static const uint32_t K[16] = {0x9E3779B1u, 0x85EBCA77u, 0xC2B2AE3Du, 0x27D4EB2Fu, 0x165667B1u, 0xD3A2646Du,
                                   0xFD7046C5u, 0xB55A4F09u, 0x6C8E9CF5u, 0x7FEB352Du, 0x846CA68Bu, 0x94D049BBu,
                                   0xBF58476Du, 0x1CE4E5B9u, 0x2545F491u, 0x9FB21C65u};
    uint32_t c[16] = {};
    if (len) memcpy(c, p, std::min<uint32_t>(len, 64u));
    uint64_t h = 0;
    for (uint32_t j = 0; j < 8; ++j) h += (uint64_t)(uint32_t)(c[2 * j] + K[2 * j]) * (uint64_t)(uint32_t)(c[2 * j + 1] + K[2 * j + 1]);
    for (uint32_t k = 64; k < len; k += 8) {
        uint64_t v = 0;
        memcpy(&v, p + k, std::min<uint32_t>(len - k, 8u));
        v *= 0x87C37B91114253D5ull;
        v = (v << 31) | (v >> 33);
        v *= 0x4CF5AD432745937Full;
        h ^= v;
        h = (h << 27) | (h >> 37);
        h = h * 5u + 0x52DCE729ull;
    }
    h ^= (uint64_t)len * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 33);
}

int tm_ptable_create(tm_engine* e, const uint8_t* topics, const uint64_t* offsets, const uint16_t* priorities, uint32_t n,
                     uint32_t default_priority, tm_ptable** table) {
    if (!e || !table || (n && (!offsets || !priorities))) return TM_EINVAL;
    auto bad_prio = [](uint32_t p) { return p > 255u && p != TM_PRIO_INFINITY; };
    if (bad_prio(default_priority))
        return einval("tm_ptable_create: default priority %u (0..255 or TM_PRIO_INFINITY)", default_priority);
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return einval("tm_ptable_create: key %u: offsets not monotone", i);
        if (offsets[i + 1] - offsets[i] > TM_MAX_TOPIC_LEN)
            return einval("tm_ptable_create: key %u of %llu bytes (over %u)", i, (unsigned long long)(offsets[i + 1] - offsets[i]),
                          (unsigned)TM_MAX_TOPIC_LEN);
        if (bad_prio(priorities[i])) return einval("tm_ptable_create: key %u: priority %u (0..255 or TM_PRIO_INFINITY)", i, priorities[i]);
    }
    if (n && offsets[n] > offsets[0] && !topics) return TM_EINVAL;
    static std::atomic<uint64_t> serials{0};
    try {
        // maps:put: a repeated key keeps its last priority
        std::unordered_map<std::string, uint16_t> map;
        std::vector<std::string> order;
        for (uint32_t i = 0; i < n; ++i) {
            std::string k(reinterpret_cast<const char*>(topics) + offsets[i], offsets[i + 1] - offsets[i]);
            auto it = map.find(k);
            if (it == map.end()) {
                order.push_back(k);
                map.emplace(std::move(k), priorities[i]);
            } else {
                it->second = priorities[i];
            }
        }
        std::vector<uint16_t> cls{(uint16_t)default_priority};
        for (const auto& kv : map) cls.push_back(kv.second);
        std::sort(cls.begin(), cls.end(), std::greater<uint16_t>());   // TM_PRIO_INFINITY = 0xFFFF sorts first
        cls.erase(std::unique(cls.begin(), cls.end()), cls.end());
        if (cls.size() > TM_PRIO_MAX_CLASSES)
            return einval("tm_ptable_create: %zu classes (distinct priorities and the default), at most %u", cls.size(),
                          (unsigned)TM_PRIO_MAX_CLASSES);
        auto class_of = [&](uint16_t p) { return (uint32_t)(std::find(cls.begin(), cls.end(), p) - cls.begin()); };
        std::unique_ptr<tm_ptable> t(new tm_ptable);
        t->e = e;
        t->serial = ++serials;
        t->ncls = (uint32_t)cls.size();
        t->dcls = class_of((uint16_t)default_priority);
        std::copy(cls.begin(), cls.end(), t->classes);
        size_t cap = 8;
        while (cap < 2 * order.size()) cap <<= 1;   // load <= 1/2
        t->slots.assign(2 * cap, 0u);
        for (const std::string& k : order) {
            const uint64_t h = prio_hash(reinterpret_cast<const uint8_t*>(k.data()), (uint32_t)k.size());
            size_t s = (uint32_t)h & (cap - 1);
            while (t->slots[2 * s + 1]) s = (s + 1) & (cap - 1);
            t->slots[2 * s] = (uint32_t)t->keys.size();
            t->slots[2 * s + 1] = PRIO_META_USED | (uint32_t)(h >> 54) << PRIO_META_HASH_SHIFT |
                                  class_of(map[k]) << PRIO_META_CLS_SHIFT | (uint32_t)k.size();
            t->keys.insert(t->keys.end(), k.begin(), k.end());
        }
        t->keys.resize(((t->keys.size() + 15) & ~(size_t)15) + 32, 0);   // the kernel's 16-B loads stay inside
        *table = t.release();
        return TM_OK;
    } catch (...) {
        return TM_ENOMEM;
    }
}

void tm_ptable_free(tm_engine* e, tm_ptable* table) {
    (void)e;
    delete table;
}

uint32_t tm_ptable_classes(const tm_ptable* table, uint16_t out[TM_PRIO_MAX_CLASSES]) {
    if (!table) return 0;
    if (out) std::copy(table->classes, table->classes + table->ncls, out);
    return table->ncls;
}

// The call's tables as one block on the device (packed again only when the
// list of tables changed), its prio entries, the batch's topic bytes, and the
// lookup kernel between lev0 and lev1.  Fills pa's inputs.
static int prio_lookup(tm_batch* b, const tm_window_prio_opts* p, PrioArgs& pa) {
    tm_batch::Prio& pr = b->prio;
    const hipStream_t stream = b->rep->stream;
    const uint32_t ntab = p->n_tables, n = b->n;
    int rc;
    std::vector<uint64_t> serials(ntab);
    uint32_t ncls = 0;
    for (uint32_t t = 0; t < ntab; ++t) {
        serials[t] = p->tables[t]->serial;
        ncls = std::max(ncls, p->tables[t]->ncls);
    }
    if (serials != pr.blk_serials || !pr.blk.d.p) {
        size_t w = (PRIO_HDR_W * (size_t)ntab + 3) & ~(size_t)3;
        std::vector<uint32_t> blk(w, 0u);
        for (uint32_t t = 0; t < ntab; ++t) {
            blk[PRIO_HDR_W * t] = (uint32_t)w;
            w += p->tables[t]->slots.size();
        }
        size_t bytes = (w * 4 + 15) & ~(size_t)15;
        for (uint32_t t = 0; t < ntab; ++t) {
            const tm_ptable& T = *p->tables[t];
            blk[PRIO_HDR_W * t + 1] = (uint32_t)bytes;
            blk[PRIO_HDR_W * t + 2] = (uint32_t)(T.slots.size() / 2 - 1);
            blk[PRIO_HDR_W * t + 3] = T.dcls;
            bytes += T.keys.size();   // (a multiple of 16)
        }
        if (bytes > 0xFFFFFFF0ull) return TM_EOVERFLOW;
        blk.resize(bytes / 4, 0u);
        for (uint32_t t = 0; t < ntab; ++t) {
            const tm_ptable& T = *p->tables[t];
            std::copy(T.slots.begin(), T.slots.end(), blk.begin() + blk[PRIO_HDR_W * t]);
            memcpy(reinterpret_cast<uint8_t*>(blk.data()) + blk[PRIO_HDR_W * t + 1], T.keys.data(), T.keys.size());
        }
        pr.blk_serials.clear();
        if ((rc = pr.blk.stage(blk.data(), blk.size(), stream))) return rc;
        pr.blk_serials = serials;
    }
    // uploaded per call, as the sessions are: acks change the queues between any two calls
    if ((rc = pr.prio.stage(reinterpret_cast<const uint32_t*>(p->prio), (size_t)p->n_prio * PRIO_SESSION_WORDS, stream)))
        return rc;
    if ((rc = pr.d_pcp.reserve(std::max<size_t>((size_t)ntab * n, 1)))) return rc;
    if ((rc = pr.lev0.create())) return rc;
    if ((rc = pr.lev1.create())) return rc;
    PrioLookupArgs la{};
    if (b->dev_tok) {
        la.bytes = b->tok.in_bytes; la.offs = b->tok.in_offs; la.base = b->tok_base;
    } else {   // tokenised on the host: the bytes go up for this call
        const size_t nbytes = b->bytes.size();
        if ((rc = pr.d_tbytes.reserve(nbytes + 32))) return rc;
        if ((rc = pr.d_toffs.reserve((size_t)n + 1))) return rc;
        if (nbytes) HIP_OK(hipMemcpyAsync(pr.d_tbytes.p, b->bytes.data(), nbytes, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(pr.d_toffs.p, b->offs.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, stream));
        la.bytes = pr.d_tbytes.p; la.offs = pr.d_toffs.p; la.base = 0;
    }
    la.blk = pr.blk.d.p; la.n = n; la.ntab = ntab; la.out = pr.d_pcp.p;
    HIP_OK(hipEventRecord(pr.lev0.e, stream));
    HIP_OK(launch_prio_lookup(la, stream));
    HIP_OK(hipEventRecord(pr.lev1.e, stream));
    pa.pcp = pr.d_pcp.p; pa.prio = pr.prio.d.p;
    pa.n = n; pa.ntab = ntab; pa.NP = p->n_prio; pa.dtab = p->default_table; pa.ncls = ncls;
    return TM_OK;
}

int tm_engine::batch_window(tm_batch* b, const tm_deliver_opts* o, const tm_window_opts* w, tm_session_window* out) {
    return batch_window_prio(b, o, w, nullptr, out, nullptr);
}

// p = nullptr: tm_batch_window, the old kernels alone.  With p but no table
// (n_tables = 0) the same kernels run and pclass / precords are filled by two
// memsets: no session has a table.
int tm_engine::batch_window_prio(tm_batch* b, const tm_deliver_opts* o, const tm_window_opts* w,
                                 const tm_window_prio_opts* p, tm_session_window* out, tm_window_prio* pout) {
    const bool device = w->flags & TM_WINDOW_DEVICE;
    if (p) *pout = tm_window_prio{};
    const uint32_t ntab = p ? p->n_tables : 0u;
    if (ntab) {   // checked before anything runs: the lookup reads the batch's topic bytes on the device
        if (!b->done) return einval("tm_batch_window_prio: the batch has not been waited for");
        if (b->tokens_only || b->bounded || (b->dev_tok ? !b->tok.in_bytes || !b->tok.in_offs : b->offs.size() != (size_t)b->n + 1))
            return einval("tm_batch_window_prio: the batch has no device copy of its topic bytes "
                          "(tm_batch_prepare_tokens): the class lookup reads them");
    }
    tm_deliver_opts dopt = *o;
    dopt.flags = (o->flags & ~TM_DELIVER_DEVICE) | (device ? TM_DELIVER_DEVICE : 0u);
    *out = tm_session_window{};
    int rc;
    if ((rc = batch_deliver(b, &dopt, &out->inboxes))) return rc;   // returns with the stream idle
    Replica& R = *b->rep;
    const hipStream_t stream = R.stream;
    tm_batch::Window& wn = b->win;
    // where batch_deliver left the result on the device, whichever copy it returned
    const bool can_drop = o->from && nl_entries > 0;
    const uint32_t* d_sub = can_drop ? b->dlv.sub.d.p : b->inbox.sub.d.p;
    const uint32_t* d_off = can_drop ? b->dlv.off.d.p : b->inbox.off.d.p;
    const uint32_t D = (uint32_t)out->inboxes.n_deliveries, nsub = out->inboxes.n_subscribers, ns = w->n_sessions;
    const size_t rr = std::max<size_t>(nsub, 1);
    const bool live = D && nsub;   // else nothing left to send: every total 0
    if ((rc = wn.disp.reserve(D))) return rc;
    if ((rc = wn.pid.reserve(D))) return rc;
    if ((rc = wn.rec.reserve(nsub))) return rc;
    tm_batch::Prio& pr = b->prio;
    if (p) {
        if ((rc = pr.pclass.reserve(D))) return rc;
        if ((rc = pr.prec.reserve((size_t)nsub * PRIO_CLASSES))) return rc;
    }
    PrioArgs pa{};
    if (live && ntab && (rc = prio_lookup(b, p, pa))) return rc;   // enqueued ahead of the window's kernels
    if (live) {
        const uint32_t ntiles = (uint32_t)(((uint64_t)D + INBOX_TILE - 1) / INBOX_TILE);
        const size_t nheads = (size_t)2 * (((size_t)D + 63) / 64);
        WindowArgs a{};
        a.nwaves = ntiles * (INBOX_TILE / 1024);
        if ((rc = wn.d_heads.reserve(nheads))) return rc;
        if ((rc = wn.d_st.reserve(rr))) return rc;
        if ((rc = wn.d_hbase.reserve(rr))) return rc;
        if ((rc = wn.d_wcount.reserve((size_t)a.nwaves + 1))) return rc;
        if ((rc = wn.d_wbs.reserve((size_t)scan_block_count(a.nwaves) + 1))) return rc;
        if ((rc = wn.d_wdisp.reserve((size_t)a.nwaves * 8))) return rc;
        if ((rc = wn.tot.reserve(2))) return rc;
        if ((rc = wn.totals.reserve(WIN_NDISP))) return rc;
        if ((rc = wn.wev0.create())) return rc;
        if ((rc = wn.wev1.create())) return rc;
        // uploaded per call: acks change the sessions on the host between any two calls
        if ((rc = wn.sess.stage(reinterpret_cast<const uint32_t*>(w->sessions), (size_t)ns * WIN_SESSION_WORDS, stream)))
            return rc;
        a.subscribers = d_sub; a.off = d_off; a.msg = b->dlv.msg.d.p; a.sess = wn.sess.d.p;
        a.D = D; a.R = nsub; a.NS = ns;
        memcpy(a.dflt, &w->defaults, sizeof a.dflt);
        a.heads = wn.d_heads.p; a.st = wn.d_st.p; a.hbase = wn.d_hbase.p;
        a.wcount = wn.d_wcount.p; a.wbs = wn.d_wbs.p; a.d_tot = wn.tot.d.p;
        a.disp = wn.disp.d.p; a.pid = wn.pid.d.p; a.rec = wn.rec.d.p;
        a.wdisp = wn.d_wdisp.p; a.totals = wn.totals.d.p;
        HIP_OK(hipMemsetAsync(wn.d_heads.p, 0, nheads * 4, stream));
        HIP_OK(hipMemsetAsync(wn.tot.d.p, 0, 8, stream));
        HIP_OK(hipEventRecord(wn.wev0.e, stream));
        if (ntab) {
            const size_t nsb = (a.nwaves + PRIO_SCAN_TILE - 1) / PRIO_SCAN_TILE;
            if ((rc = pr.d_ptab.reserve(rr))) return rc;
            if ((rc = pr.d_chbase.reserve(rr * PRIO_CLASSES))) return rc;
            if ((rc = pr.d_cw.reserve(((size_t)a.nwaves + 1) * PRIO_CLASSES))) return rc;
            if ((rc = pr.d_cbs.reserve((nsb + 1) * PRIO_CLASSES))) return rc;
            if ((rc = pr.d_ctot.reserve(PRIO_CLASSES))) return rc;
            if ((rc = pr.d_cthr.reserve(rr * PRIO_CLASSES))) return rc;
            pa.publishes = can_drop ? b->dlv.pub.d.p : b->inbox.pub.d.p;
            pa.ptab = pr.d_ptab.p; pa.chbase = pr.d_chbase.p; pa.cw = pr.d_cw.p; pa.cbs = pr.d_cbs.p;
            pa.ctot = pr.d_ctot.p; pa.cthr = pr.d_cthr.p; pa.prec = pr.prec.d.p; pa.pclass = pr.pclass.d.p;
            HIP_OK(launch_window_prio(a, pa, stream));
        } else {
            HIP_OK(launch_window(a, stream));
            if (p) {   // no table: no class anywhere
                HIP_OK(hipMemsetAsync(pr.pclass.d.p, 0xFF, D, stream));
                HIP_OK(hipMemsetAsync(pr.prec.d.p, 0, (size_t)nsub * PRIO_CLASSES * sizeof(uint2), stream));
            }
        }
        HIP_OK(hipEventRecord(wn.wev1.e, stream));
        if ((rc = wn.tot.fetch(2, stream))) return rc;
        if ((rc = wn.totals.fetch(WIN_NDISP, stream))) return rc;
    }
    if (!device) {
        if ((rc = wn.disp.fetch(live ? D : 0, stream))) return rc;
        if ((rc = wn.pid.fetch(live ? D : 0, stream))) return rc;
        if ((rc = wn.rec.fetch(live ? nsub : 0, stream))) return rc;
        if (p) {
            if ((rc = pr.pclass.fetch(live ? D : 0, stream))) return rc;
            if ((rc = pr.prec.fetch(live ? (size_t)nsub * PRIO_CLASSES : 0, stream))) return rc;
        }
    }
    if (p) {
        pout->pclass = pr.pclass.view(device);
        pout->precords = (const tm_prio_record*)pr.prec.view(device);
    }
    out->disp = wn.disp.view(device);
    out->packet_ids = wn.pid.view(device);
    out->records = (const tm_window_record*)wn.rec.view(device);
    if (!live) return TM_OK;
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipEventElapsedTime(&out->kernel_ms, wn.wev0.e, wn.wev1.e));
    if (ntab) HIP_OK(hipEventElapsedTime(&pout->lookup_kernel_ms, pr.lev0.e, pr.lev1.e));
    const char* fn = p ? "tm_batch_window_prio" : "tm_batch_window";
    if (wn.tot.h.p[1]) {
        snprintf(last_error(), 512, "%s: %u indices past %u deliveries, %u inboxes or %u sessions", fn, wn.tot.h.p[1],
                 D, nsub, ns);
        return TM_EIO;
    }
    uint64_t sum = 0;
    for (uint32_t k = 0; k < WIN_NDISP; ++k) sum += out->totals[k] = wn.totals.h.p[k];
    if (sum != D) {
        snprintf(last_error(), 512, "%s: dispositions of %llu of %u deliveries", fn, (unsigned long long)sum, D);
        return TM_EIO;
    }
    return TM_OK;
}

int tm_engine::rules_match(Replica& R, const uint8_t* names, const uint64_t* noffs, uint32_t n, const uint8_t* rules,
                const uint64_t* roffs, uint32_t r, bool dollar_rule, uint32_t* bits) {
    const hipStream_t stream = R.stream;
    WordDict rd;
    std::vector<TWord> ws;
    std::vector<uint32_t> rw, ro(1, 0), nw, no(1, 0);
    std::vector<uint8_t> rf(r), nf(n);
    auto id_of = [](const TWord& w) -> uint32_t {
        return w.n == 0 ? W_EMPTY : is_plus(w) ? W_PLUS : is_hash(w) ? W_HASH : W_UNKNOWN;
    };
    for (uint32_t j = 0; j < r; ++j) {
        const uint8_t* p = rules + roffs[j];
        const size_t len = roffs[j + 1] - roffs[j];
        split_words(p, len, ws);
        for (const TWord& w : ws) {
            uint32_t id = id_of(w);
            if (id == W_UNKNOWN) id = rd.intern(w.p, w.n);
            rw.push_back(id);
        }
        ro.push_back((uint32_t)rw.size());
        rf[j] = (len > 0 && (p[0] == '+' || p[0] == '#')) ? 1 : 0;
    }
    for (uint32_t t = 0; t < n; ++t) {
        const uint8_t* p = names + noffs[t];
        const size_t len = noffs[t + 1] - noffs[t];
        split_words(p, len, ws);
        for (const TWord& w : ws) {
            uint32_t id = id_of(w);
            if (id == W_UNKNOWN) id = rd.find(w.p, w.n);
            nw.push_back(id);
        }
        if (nw.size() > 0xFFFFFFF0ull) return TM_EOVERFLOW;
        no.push_back((uint32_t)nw.size());
        nf[t] = (len > 0 && p[0] == '$') ? 1 : 0;
    }
    const uint32_t wpr = (r + 31) / 32;
    // one device block: [rw | ro | nw | no | bits] in u32, then rf | nf bytes
    const size_t nbits = (size_t)n * wpr;
    const size_t words = rw.size() + ro.size() + nw.size() + no.size() + nbits + (r + n + 3) / 4 + 4;
    int rc;
    if ((rc = R.tab.d_rl.reserve(words))) return rc;
    uint32_t* d = R.tab.d_rl.p;
    uint32_t *d_rw = d, *d_ro = d_rw + rw.size(), *d_nw = d_ro + ro.size(), *d_no = d_nw + nw.size();
    uint32_t* d_bits = d_no + no.size();
    uint8_t* d_rf = reinterpret_cast<uint8_t*>(d_bits + nbits);
    uint8_t* d_nf = d_rf + r;
    HIP_OK(hipMemcpyAsync(d_rw, rw.data(), rw.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_ro, ro.data(), ro.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_nw, nw.data(), nw.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_no, no.data(), no.size() * 4, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_rf, rf.data(), r, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(d_nf, nf.data(), n, hipMemcpyHostToDevice, stream));
    RulesArgs a{};
    a.nwords = d_nw; a.noff = d_no; a.nflag = d_nf; a.n = n;
    a.rwords = d_rw; a.roff = d_ro; a.rflag = d_rf; a.r = r;
    a.dollar_rule = dollar_rule ? 1u : 0u; a.wpr = wpr; a.bits = d_bits;
    HIP_OK(launch_rules_match(a, stream));
    HIP_OK(hipMemcpyAsync(bits, d_bits, nbits * 4, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));   // the host vectors above are freed on return
    return TM_OK;
}
