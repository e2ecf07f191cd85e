// tm_acl.cpp -- batched ACL check (emqx_access_control:check_acl/3): the host
// compiler of a rule list into the flat block the kernel reads (layout in
// tm_internal.hpp), its upload to every replica, and the dispatch of a
// request batch (tm_acl_check).
#include "tm_engine_impl.hpp"

#include <memory>

struct tm_acl {
    tm_engine* e = nullptr;
    uint32_t n_rules = 0;
    std::vector<uint32_t> blk;   // words, then the bytes (padded to a word)
    // per replica: the block's copy in HBM and the buffers of one check call
    // (calls on one engine are serialised by its mutex)
    struct Dev {
        DevBuf<uint32_t> d_blk;
        DevBuf<uint8_t> d_buf;
        PinBuf<uint8_t> h_buf;   // pinned: the call's inputs packed for one copy, then its outputs
        Event ev0, ev1;
        float ms = 0.f;
    };
    std::vector<Dev> dev;
    float last_ms = 0.f;
};

namespace {

int einval(const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
    snprintf(last_error(), 512, fmt, a, b);
    return TM_EINVAL;
}

struct AclCompiler {
    std::vector<uint32_t> w;       // block words
    std::vector<uint8_t> bytes;    // block bytes (follow the words)
    std::vector<size_t> fix;       // words holding a byte offset: + 4 * w.size() at the end

    uint32_t put_bytes(const uint8_t* p, size_t n) {
        const uint32_t off = (uint32_t)bytes.size();
        if (n) bytes.insert(bytes.end(), p, p + n);
        return off;
    }

    // node `at` of the pre-order array -> its postfix ops; returns the index
    // after its subtree, or a negative TM_E* code
    long who(const tm_acl_who* ws, uint32_t n, uint32_t at, uint32_t depth, uint32_t rule) {
        if (at >= n) return einval("rule %llu: who array ends inside a tree", rule);
        if (depth > TM_ACL_MAX_WHO_DEPTH)
            return einval("rule %llu: who nested deeper than %llu", rule, TM_ACL_MAX_WHO_DEPTH);
        const tm_acl_who& x = ws[at];
        switch (x.kind) {
        case TM_WHO_ALL:
        case TM_WHO_CLIENT_ALL:
        case TM_WHO_USER_ALL:
            w.push_back(ACL_OP_TRUE);
            return at + 1;
        case TM_WHO_CLIENT:
        case TM_WHO_USER:
            if (x.val_len && !x.val) return einval("rule %llu: who node %llu has no value", rule, at);
            if (x.val_len >= (1u << 28)) return einval("rule %llu: who value too long", rule);
            w.push_back((x.kind == TM_WHO_CLIENT ? ACL_OP_CLIENT : ACL_OP_USER) | (x.val_len << 4));
            fix.push_back(w.size());
            w.push_back(put_bytes(x.val, x.val_len));
            return at + 1;
        case TM_WHO_IPADDR: {
            if (x.family != 4 && x.family != 6)
                return einval("rule %llu: ipaddr family %llu is not 4 or 6", rule, x.family);
            w.push_back(ACL_OP_IPADDR | ((uint32_t)x.family << 4));
            const size_t nb = x.family == 4 ? 4 : 16;
            for (const uint8_t* a : {x.lo, x.hi})
                for (size_t q = 0; q < 4; ++q) {
                    uint32_t v = 0;
                    for (size_t b = 0; b < 4; ++b) v = (v << 8) | (4 * q + b < nb ? a[4 * q + b] : 0u);
                    w.push_back(v);
                }
            return at + 1;
        }
        case TM_WHO_AND:
        case TM_WHO_OR: {
            const bool is_and = x.kind == TM_WHO_AND;
            w.push_back(is_and ? ACL_OP_TRUE : ACL_OP_FALSE);   // {'and', []} = true, {'or', []} = false
            uint32_t next = at + 1;
            for (uint32_t c = 0; c < x.n_children; ++c) {
                const long r = who(ws, n, next, depth + 1, rule);
                if (r < 0) return r;
                next = (uint32_t)r;
                w.push_back(is_and ? ACL_OP_AND : ACL_OP_OR);
            }
            return next;
        }
        default:
            return einval("rule %llu: unknown who kind %llu", rule, x.kind);
        }
    }

    int topic(const tm_acl_topic& t, size_t entry, uint32_t rule) {
        if (t.len > TM_MAX_TOPIC_LEN) return einval("rule %llu: filter of %llu bytes", rule, t.len);
        if (t.len && !t.filter) return einval("rule %llu: filter without bytes", rule);
        if (t.eq > 1) return einval("rule %llu: eq flag %llu", rule, t.eq);
        fix.push_back(entry);
        w[entry] = put_bytes(t.filter, t.len);
        w[entry + 1] = t.len | (t.eq ? ACL_EQ : 0u);
        w[entry + 2] = (uint32_t)w.size();
        uint32_t nlev = 0;
        if (!t.eq) {   // emqx_topic:words/1 of a compiled filter (src/emqx_access_rule.erl:72-77)
            uint32_t s = 0;
            for (uint32_t i = 0; i <= t.len; ++i) {
                if (i < t.len && t.filter[i] != '/') continue;
                const uint8_t* p = t.filter + s;
                const uint32_t l = i - s;
                uint32_t kind = ACL_L_LIT;
                if (l == 1 && p[0] == '+') kind = ACL_L_PLUS;
                else if (l == 1 && p[0] == '#') kind = ACL_L_HASH;
                else if (l == 2 && p[0] == '%' && p[1] == 'c') kind = ACL_L_VARC;
                else if (l == 2 && p[0] == '%' && p[1] == 'u') kind = ACL_L_VARU;
                w.push_back(s | (l << ACL_L_LEN_SHIFT) | (kind << ACL_L_KIND_SHIFT) | (i == t.len ? ACL_L_LAST : 0u));
                ++nlev;
                s = i + 1;
            }
        }
        w[entry + 3] = nlev;
        return TM_OK;
    }

    int run(const tm_acl_rule* rules, uint32_t n, std::vector<uint32_t>& out) {
        w.assign(ACL_HDR + (size_t)ACL_RULE_W * n, 0u);
        w[0] = n;
        for (uint32_t j = 0; j < n; ++j) {
            const tm_acl_rule& r = rules[j];
            if (r.allow > 1) return einval("rule %llu: allow %llu", j, r.allow);
            if (r.access > 3) return einval("rule %llu: access %llu", j, r.access);
            const size_t rw = ACL_HDR + (size_t)ACL_RULE_W * j;
            w[rw] = r.allow | (r.access << 8) | (r.access == 0 ? 1u << 16 : 0u);
            if (r.access == 0) continue;   // {A, all}
            if (!r.who || !r.n_who) return einval("rule %llu: no who", j);
            if (r.n_topics && !r.topics) return einval("rule %llu: no topics array", j);
            w[rw + 1] = (uint32_t)w.size();
            const long end = who(r.who, r.n_who, 0, 1, j);
            if (end < 0) return (int)end;
            if ((uint32_t)end != r.n_who)
                return einval("rule %llu: who array holds more than one tree (%llu nodes left)", j, r.n_who - end);
            w[rw + 2] = (uint32_t)w.size() - w[rw + 1];
            const size_t tt = w.size();
            w[rw + 3] = (uint32_t)tt;
            w[rw + 4] = r.n_topics;
            w.resize(tt + (size_t)ACL_TOPIC_W * r.n_topics, 0u);
            for (uint32_t f = 0; f < r.n_topics; ++f) {
                const int rc = topic(r.topics[f], tt + (size_t)ACL_TOPIC_W * f, j);
                if (rc) return rc;
            }
            if (w.size() + bytes.size() / 4 > 0x3FFFFFFFull) return TM_EOVERFLOW;
        }
        const uint32_t base = (uint32_t)(w.size() * 4);
        for (size_t i : fix) w[i] += base;
        out = w;
        out.resize(w.size() + (bytes.size() + 3) / 4 + 1, 0u);
        if (!bytes.empty()) memcpy(out.data() + w.size(), bytes.data(), bytes.size());
        return TM_OK;
    }
};

size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// one slice [lo, hi) of the requests on replica R
int acl_slice(tm_acl* acl, Replica& R, const tm_acl_clients* cl, const uint8_t* topics, const uint64_t* offsets,
              const uint32_t* client_of, const uint8_t* access, uint32_t lo, uint32_t hi, uint8_t* verdict,
              uint32_t* rule) {
    tm_acl::Dev& D = acl->dev[R.index];
    const uint32_t n = hi - lo, m = cl->m;
    const uint64_t base = offsets[lo], nbytes = offsets[hi] - base;
    const uint64_t cbytes = m ? cl->clientid_offsets[m] : 0, ubytes = m ? cl->username_offsets[m] : 0;
    // inputs, each section 16-B aligned: name bytes (+ 16 B the staging loads may touch) | offsets | client_of |
    // access | client ids | their offsets | user names | their offsets | flags | family | peerhost; then the outputs
    size_t o = 0;
    const size_t o_top = o;  o = up16(o + nbytes + 16);
    const size_t o_off = o;  o = up16(o + ((size_t)n + 1) * 8);
    const size_t o_cof = o;  o = up16(o + (size_t)n * 4);
    const size_t o_acc = o;  o = up16(o + n);
    const size_t o_cid = o;  o = up16(o + cbytes);
    const size_t o_cio = o;  o = up16(o + ((size_t)m + 1) * 8);
    const size_t o_usr = o;  o = up16(o + ubytes);
    const size_t o_uso = o;  o = up16(o + ((size_t)m + 1) * 8);
    const size_t o_flg = o;  o = up16(o + m);
    const size_t o_fam = o;  o = up16(o + m);
    const size_t o_peer = o; o = up16(o + (size_t)m * 16);
    const size_t in_bytes = o;
    const size_t o_rule = o; o = up16(o + (size_t)n * 4);
    const size_t o_ver = o;  o = up16(o + n);
    const size_t total = o;
    int rc;
    if ((rc = D.d_buf.reserve(total))) return rc;
    if ((rc = D.h_buf.reserve(total))) return rc;
    uint8_t* h = D.h_buf.p;
    if (nbytes) memcpy(h + o_top, topics + base, nbytes);
    memset(h + o_top + nbytes, 0, 16);
    memcpy(h + o_off, offsets + lo, ((size_t)n + 1) * 8);
    memcpy(h + o_cof, client_of + lo, (size_t)n * 4);
    memcpy(h + o_acc, access + lo, n);
    const uint64_t zero = 0;
    if (cbytes) memcpy(h + o_cid, cl->clientids, cbytes);
    memcpy(h + o_cio, m ? cl->clientid_offsets : &zero, ((size_t)m + 1) * 8);
    if (ubytes) memcpy(h + o_usr, cl->usernames, ubytes);
    memcpy(h + o_uso, m ? cl->username_offsets : &zero, ((size_t)m + 1) * 8);
    if (m) {
        memcpy(h + o_flg, cl->flags, m);
        memcpy(h + o_fam, cl->family, m);
        memcpy(h + o_peer, cl->peerhost, (size_t)m * 16);
    }
    const hipStream_t s = R.stream;
    uint8_t* d = D.d_buf.p;
    HIP_OK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, s));
    AclArgs a{};
    a.blk = D.d_blk.p;
    a.n_rules = acl->n_rules;
    a.topics = d + o_top;
    a.offs = reinterpret_cast<const uint64_t*>(d + o_off);
    a.base = base;
    a.client_of = reinterpret_cast<const uint32_t*>(d + o_cof);
    a.access = d + o_acc;
    a.n = n;
    a.cid = d + o_cid;
    a.cid_off = reinterpret_cast<const uint64_t*>(d + o_cio);
    a.usr = d + o_usr;
    a.usr_off = reinterpret_cast<const uint64_t*>(d + o_uso);
    a.cflags = d + o_flg;
    a.cfamily = d + o_fam;
    a.peer = reinterpret_cast<const uint4*>(d + o_peer);
    a.verdict = d + o_ver;
    a.rule = reinterpret_cast<uint32_t*>(d + o_rule);
    HIP_OK(hipEventRecord(D.ev0.e, s));
    HIP_OK(launch_acl_check(a, s));
    HIP_OK(hipEventRecord(D.ev1.e, s));
    HIP_OK(hipMemcpyAsync(h + o_rule, d + o_rule, total - o_rule, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipEventElapsedTime(&D.ms, D.ev0.e, D.ev1.e));
    memcpy(rule + lo, h + o_rule, (size_t)n * 4);
    memcpy(verdict + lo, h + o_ver, n);
    return TM_OK;
}

}  // namespace

int tm_acl_create(tm_engine* e, const tm_acl_rule* rules, uint32_t n, tm_acl** out) {
    if (!e || !out || (n && !rules)) return TM_EINVAL;
    try {
        std::unique_ptr<tm_acl> acl(new tm_acl);
        acl->e = e;
        acl->n_rules = n;
        AclCompiler c;
        int rc = c.run(rules, n, acl->blk);
        if (rc) return rc;
        acl->dev.resize(e->reps.size());
        for (size_t i = 0; i < e->reps.size() && !rc; ++i) {
            tm_acl::Dev& D = acl->dev[i];
            rc = [&]() -> int {
                HIP_OK(hipSetDevice(e->reps[i]->device));
                int r;
                if ((r = D.d_blk.alloc(acl->blk.size()))) return r;
                HIP_OK(hipMemcpy(D.d_blk.p, acl->blk.data(), acl->blk.size() * 4, hipMemcpyHostToDevice));
                if ((r = D.ev0.create())) return r;
                return D.ev1.create();
            }();
        }
        if (!e->reps.empty()) (void)e->set_device();
        if (rc) {
            tm_acl_free(e, acl.release());
            return rc;
        }
        *out = acl.release();
        return TM_OK;
    } catch (...) {
        return TM_ENOMEM;
    }
}

void tm_acl_free(tm_engine* e, tm_acl* acl) {
    if (!acl) return;
    (void)e;
    for (size_t i = 0; i < acl->dev.size(); ++i) {
        if (i < acl->e->reps.size()) (void)hipSetDevice(acl->e->reps[i]->device);
        acl->dev[i] = {};
    }
    if (!acl->dev.empty()) (void)acl->e->set_device();
    delete acl;
}

int tm_acl_check(tm_engine* e, tm_acl* acl, const tm_acl_clients* clients, const uint8_t* topics,
                 const uint64_t* offsets, const uint32_t* client_of, const uint8_t* access, uint32_t n,
                 uint8_t* verdict, uint32_t* rule) {
    if (!e || !acl || acl->e != e) return TM_EINVAL;
    if (e->reps.empty()) return TM_ENODEV;   // host-only engine: no CPU fallback
    if (!n) return TM_OK;
    if (!clients || !offsets || !client_of || !access || !verdict || !rule) return TM_EINVAL;
    const uint32_t m = clients->m;
    if (m && (!clients->clientid_offsets || !clients->username_offsets || !clients->flags || !clients->family ||
              !clients->peerhost))
        return TM_EINVAL;
    for (uint32_t c = 0; c < m; ++c) {
        if (clients->clientid_offsets[c + 1] < clients->clientid_offsets[c] ||
            clients->username_offsets[c + 1] < clients->username_offsets[c])
            return einval("client %llu: offsets not monotone", c);
        const uint8_t f = clients->family[c];
        if (f != 0 && f != 4 && f != 6) return einval("client %llu: family %llu", c, f);
    }
    if (m && ((clients->clientid_offsets[m] && !clients->clientids) ||
              (clients->username_offsets[m] && !clients->usernames)))
        return TM_EINVAL;
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > TM_MAX_TOPIC_LEN)
            return einval("request %llu: name longer than %llu bytes (or offsets not monotone)", i, TM_MAX_TOPIC_LEN);
        if (client_of[i] >= m) return einval("request %llu: client %llu out of range", i, client_of[i]);
        if (access[i] != TM_ACL_PUBLISH && access[i] != TM_ACL_SUBSCRIBE)
            return einval("request %llu: access %llu", i, access[i]);
    }
    if (offsets[n] > offsets[0] && !topics) return TM_EINVAL;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    int rc = e->set_device();
    if (rc) return rc;
    // as tm_rules_match: a big batch is cut into one contiguous slice per replica
    const size_t k = (e->reps.size() > 1 && n >= 65536) ? e->reps.size() : 1;
    std::vector<int> rcs(k, TM_OK);
    auto one = [&](size_t i, Replica& R) {
        const uint32_t lo = tm_engine::slice_lo(n, k, i), hi = tm_engine::slice_lo(n, k, i + 1);
        if (hipSetDevice(R.device) != hipSuccess) { rcs[i] = TM_EIO; return; }
        try {
            rcs[i] = acl_slice(acl, R, clients, topics, offsets, client_of, access, lo, hi, verdict, rule);
        } catch (...) {
            rcs[i] = TM_ENOMEM;
        }
    };
    float ms = 0.f;
    if (k == 1) {
        Replica& R = e->pick();
        one(0, R);
        ms = acl->dev[R.index].ms;
    } else {
        std::vector<std::thread> th;
        for (size_t i = 0; i < k; ++i) th.emplace_back([&, i] { one(i, *e->reps[i]); });
        for (auto& t : th) t.join();
        for (size_t i = 0; i < k; ++i) ms = std::max(ms, acl->dev[i].ms);
    }
    acl->last_ms = ms;
    (void)e->set_device();
    for (int x : rcs)
        if (x) return x;
    return TM_OK;
}

float tm_acl_kernel_ms(tm_engine* e, tm_acl* acl) {
    if (!e || !acl || acl->e != e) return 0.f;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    return acl->last_ms;
}
