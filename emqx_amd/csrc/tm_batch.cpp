// tm_batch.cpp -- batches: tokenise (host or device), byte-level dedup, upload,
// launch of the walk, wait / capacity relaunch, the dense CSR and samples.
// The device side is tm_kernels.hip; the path is src/emqx_router.erl:127-133.
#include "tm_engine_impl.hpp"

int tm_engine::ensure_slow_scratch(tm_batch* b) {
    int rc;
    if (!b->s_waves) {
        // one wave per generic-path topic at a time, latency-bound: a
        // skewed batch (C5: ~28k rows of ~1,000 matches) needs several
        // waves per CU; idle waves exit at once (scratch ~350 KB each)
        uint32_t w = b->n < 65536 ? 64u : std::min<uint32_t>(TM_SLOW_WAVES_MAX, b->n / 32);
        b->s_waves = w;
    }
    const size_t q = (size_t)b->s_waves * b->s_qcap, o = (size_t)b->s_waves * b->s_ocap;
    if ((rc = b->gen.d_sqpar.reserve(q))) return rc;
    if ((rc = b->gen.d_sqpw.reserve(q))) return rc;
    if ((rc = b->gen.d_sqmeta.reserve(q))) return rc;
    if ((rc = b->gen.d_sqkey.reserve(q))) return rc;
    if ((rc = b->gen.d_sofid.reserve(o))) return rc;
    if ((rc = b->gen.d_sokey.reserve(o))) return rc;
    return TM_OK;
}

void tm_engine::tokenize_range(const TokView& v, uint32_t lo, uint32_t hi, std::vector<uint32_t>& slow_out) const {
    std::vector<TWord> ws;
    for (uint32_t t = lo; t < hi; ++t) {
        const uint8_t* p = v.bytes + v.offs[t];
        const size_t len = v.offs[t + 1] - v.offs[t];
        split_words(p, len, ws);
        uint32_t* out = v.words + v.toff[t];
        bool irregular = false;
        for (size_t i = 0; i < ws.size(); ++i) {
            const TWord& w = ws[i];
            const uint32_t cls = word_class(w, irregular);
            uint32_t id;
            if (w.n == 0) id = W_EMPTY;
            else if (is_plus(w)) id = W_PLUS;
            else if (is_hash(w)) id = W_HASH;
            else id = dict.find(w.p, w.n);
            out[i] = (cls << WID_BITS) | id;
        }
        uint8_t fl = 0;
        if (len > 0 && p[0] == '$') fl |= TF_DOLLAR;
        if (irregular || ws.size() > FAST_MAX_DEPTH) fl |= TF_SLOW;
        v.tflags[t] = fl;
        if (fl & TF_SLOW) slow_out.push_back(t);
    }
}

int tm_engine::count_words(const uint8_t* bytes, const uint64_t* offs, uint32_t n, uint32_t* toff, uint64_t* total) {
    uint64_t acc = 0;
    for (uint32_t t = 0; t < n; ++t) {
        toff[t] = (uint32_t)acc;
        const uint8_t* p = bytes + offs[t];
        const size_t len = offs[t + 1] - offs[t];
        acc += 1 + (uint64_t)std::count(p, p + len, (uint8_t)'/');
        if (acc > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    }
    toff[n] = (uint32_t)acc;
    *total = acc;
    return TM_OK;
}

void tm_engine::tokenize_view(const TokView& v, uint32_t n, std::vector<uint32_t>& slow_all) const {
    slow_all.clear();
    const unsigned nt = (n >= 65536) ? threads : 1;
    if (nt <= 1) {
        tokenize_range(v, 0, n, slow_all);
        return;
    }
    std::vector<std::vector<uint32_t>> slow(nt);
    std::vector<std::thread> th;
    for (unsigned i = 0; i < nt; ++i) {
        const uint32_t lo = (uint32_t)((uint64_t)n * i / nt), hi = (uint32_t)((uint64_t)n * (i + 1) / nt);
        th.emplace_back([this, &v, lo, hi, &slow, i] { tokenize_range(v, lo, hi, slow[i]); });
    }
    for (auto& x : th) x.join();
    for (auto& s : slow) slow_all.insert(slow_all.end(), s.begin(), s.end());
}

int tm_engine::tokenize(tm_batch* b) {
    const uint32_t n = b->n;
    b->h_toff.resize((size_t)n + 1);
    b->h_tflags.resize(n);
    uint64_t acc = 0;
    int rc = count_words(b->bytes.data(), b->offs.data(), n, b->h_toff.data(), &acc);
    if (rc) return rc;
    b->nwords = acc;
    b->h_words.resize(acc ? acc : 1);
    TokView v{b->bytes.data(), b->offs.data(), b->h_words.data(), b->h_toff.data(), b->h_tflags.data()};
    tokenize_view(v, n, b->h_slow);
    b->dict_size = dict.size();
    return TM_OK;
}

int tm_engine::tokenize_into(const uint8_t* bytes, const uint64_t* offs, uint32_t n, uint32_t* words, uint64_t cap,
                  uint32_t* toff, uint8_t* tflags, uint64_t* nwords) {
    uint64_t acc = 0;
    int rc = count_words(bytes, offs, n, toff, &acc);
    if (rc) return rc;
    *nwords = acc;
    if (acc > cap) return TM_EOVERFLOW;
    std::vector<uint32_t> slow;
    TokView v{bytes, offs, words, toff, tflags};
    tokenize_view(v, n, slow);
    return TM_OK;
}

int tm_engine::upload_batch(tm_batch* b) {
    int rc;
    const uint32_t n = b->n;
    if ((rc = b->tok.d_words.reserve(b->h_words.size()))) return rc;
    if ((rc = b->tok.d_toff.reserve((size_t)n + 1))) return rc;
    if ((rc = b->tok.d_tflags.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_slow.reserve(std::max<size_t>(b->h_slow.size(), 1)))) return rc;
    const hipStream_t S = st(b);
    HIP_OK(hipMemcpyAsync(b->tok.d_words.p, b->h_words.data(), b->h_words.size() * 4, hipMemcpyHostToDevice, S));
    HIP_OK(hipMemcpyAsync(b->tok.d_toff.p, b->h_toff.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, S));
    if (n) HIP_OK(hipMemcpyAsync(b->tok.d_tflags.p, b->h_tflags.data(), n, hipMemcpyHostToDevice, S));
    if (!b->h_slow.empty())
        HIP_OK(hipMemcpyAsync(b->tok.d_slow.p, b->h_slow.data(), b->h_slow.size() * 4, hipMemcpyHostToDevice, S));
    b->dev_slow = false;
    return reserve_outputs(b);
}

int tm_engine::tokenize_device(const uint8_t* topics, const uint64_t* offsets, uint32_t n, uint32_t* d_words, uint64_t cap,
                    uint32_t* d_toff, uint8_t* d_tflags, uint64_t* nwords, const TokStaged* st,
                    uint64_t st_base, uint64_t st_nbytes, uint64_t off_item0) {
    if (reps.empty()) return TM_ENODEV;
    int rc;
    Replica& R = *reps[0];   // the caller's device buffers are on the first replica's device
    const hipStream_t stream = R.stream;
    tm_batch* b = &R.tokb;
    const uint64_t base = st ? st_base : offsets[0], nbytes = st ? st_nbytes : offsets[n] - base;
    if (nbytes + n + 1 > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    if ((rc = sync_device(&R))) return rc;
    if ((rc = b->tok.d_bytes.reserve(nbytes + 16))) return rc;
    if ((rc = b->tok.d_boffs.reserve((size_t)n + 1))) return rc;
    if ((rc = b->tok.d_wcount.reserve((size_t)n + 2))) return rc;   // per tile + total
    if ((rc = b->tok.d_slow.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_nslow.reserve(2))) return rc;
    if ((rc = b->dcsr.d_bsums.reserve((size_t)scan_block_count(n) + 1))) return rc;
    if ((rc = b->dcsr.h_total.reserve(4))) return rc;
    if (st) {
        // each staged chunk crosses as soon as it is in place; the chunks
        // are cut at the staging's own item bounds, so a chunk never waits
        // for more than the items it covers
        auto wait_item = [&](uint64_t item) {
            while (!__atomic_load_n(st->ready + item, __ATOMIC_ACQUIRE)) std::this_thread::yield();
        };
        for (uint64_t lo = base; lo < base + nbytes;) {
            const uint64_t item = lo / st->chunk_bytes, hi = std::min(base + nbytes, (item + 1) * st->chunk_bytes);
            wait_item(item);
            HIP_OK(hipMemcpyAsync(b->tok.d_bytes.p + (lo - base), topics + lo, hi - lo, hipMemcpyHostToDevice, stream));
            lo = hi;
        }
        for (uint64_t lo = 0; lo <= n;) {
            const uint64_t g = off_item0 + lo, item = g / st->chunk_offs;
            const uint64_t hi = std::min<uint64_t>((uint64_t)n + 1, (item + 1) * st->chunk_offs - off_item0);
            wait_item(st->nbyte_items + item);
            HIP_OK(hipMemcpyAsync(b->tok.d_boffs.p + lo, offsets + lo, (hi - lo) * 8, hipMemcpyHostToDevice, stream));
            lo = hi;
        }
        if (__atomic_load_n(st->bad, __ATOMIC_ACQUIRE)) {   // (checked before any kernel reads the offsets)
            HIP_OK(hipStreamSynchronize(stream));
            return TM_EINVAL;
        }
    } else {
        if (nbytes) HIP_OK(hipMemcpyAsync(b->tok.d_bytes.p, topics + base, nbytes, hipMemcpyHostToDevice, stream));
        HIP_OK(hipMemcpyAsync(b->tok.d_boffs.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, stream));
    }
    if (!n) HIP_OK(hipMemsetAsync(d_toff, 0, 4, stream));
    TokArgs t{};
    t.bytes = b->tok.d_bytes.p; t.offs = b->tok.d_boffs.p; t.base = base; t.n = n;
    t.keys = R.tab.d_dkey.p; t.tails = R.tab.d_tail.p; t.dict_mask = R.d_dict_n - 1; t.arena = R.tab.d_arena.p;
    t.wcount = b->tok.d_wcount.p; t.tflags = d_tflags; t.toff = d_toff; t.words = d_words; t.words_cap = cap;
    t.slow_list = b->tok.d_slow.p; t.d_nslow = b->tok.d_nslow.p;
    t.tile_topics = tok_tile_topics(n, nbytes);
    ScanArgs ts{};
    ts.block_sums = b->dcsr.d_bsums.p;
    HIP_OK(launch_tokenize(t, ts, b->tok.d_nslow.p + 1, stream));
    HIP_OK(hipMemcpyAsync(b->dcsr.h_total.p, b->tok.d_nslow.p + 1, 4, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    *nwords = n ? b->dcsr.h_total.p[0] : 0;
    return *nwords > cap ? TM_EOVERFLOW : TM_OK;
}

int tm_engine::prepare_tokens(tm_batch* b, const uint32_t* words, const uint32_t* toff, const uint8_t* tflags, uint32_t n,
                   uint64_t nwords, bool on_device) {
    if (nwords > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    const hipStream_t stream = b->rep ? st(b) : nullptr;   // (host-only engine: none)
    b->n = n;
    b->nwords = nwords;
    b->tokens_only = true;
    b->dev_tok = false;
    b->launched = b->done = false;
    b->bytes.clear();
    b->offs.clear();
    int rc;
    if (!on_device) {
        if (toff[0] != 0 || toff[n] != nwords) return TM_EINVAL;
        b->h_slow.clear();
        for (uint32_t t = 0; t < n; ++t) {
            const uint8_t f = tflags[t];
            if (toff[t + 1] < toff[t] || (f & ~(TF_DOLLAR | TF_SLOW))) return TM_EINVAL;
            if (toff[t + 1] - toff[t] > FAST_MAX_DEPTH && !(f & TF_SLOW)) return TM_EINVAL;
            if (f & TF_SLOW) b->h_slow.push_back(t);
        }
        b->h_words.assign(words, words + nwords);
        if (b->h_words.empty()) b->h_words.push_back(0);
        b->h_toff.assign(toff, toff + (size_t)n + 1);
        b->h_tflags.assign(tflags, tflags + n);
        if (device < 0) return TM_OK;
        return upload_batch(b);
    }
    if (device < 0) return TM_ENODEV;
    b->h_words.clear(); b->h_toff.clear(); b->h_tflags.clear(); b->h_slow.clear();
    if ((rc = b->tok.d_words.reserve(std::max<uint64_t>(nwords, 1)))) return rc;
    if ((rc = b->tok.d_toff.reserve((size_t)n + 1))) return rc;
    if ((rc = b->tok.d_tflags.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_slow.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_nslow.reserve(2))) return rc;
    if ((rc = b->tok.h_bad.reserve(2))) return rc;
    if (nwords) HIP_OK(hipMemcpyAsync(b->tok.d_words.p, words, nwords * 4, hipMemcpyDeviceToDevice, stream));
    HIP_OK(hipMemcpyAsync(b->tok.d_toff.p, toff, ((size_t)n + 1) * 4, hipMemcpyDeviceToDevice, stream));
    if (n) HIP_OK(hipMemcpyAsync(b->tok.d_tflags.p, tflags, n, hipMemcpyDeviceToDevice, stream));
    HIP_OK(hipMemsetAsync(b->tok.d_nslow.p, 0, 2 * 4, stream));
    // toff[0] and toff[n] checked with the rest: a walk must never read past words[]
    HIP_OK(launch_token_check(b->tok.d_toff.p, b->tok.d_tflags.p, n, nwords, b->tok.d_slow.p, b->tok.d_nslow.p,
                              b->tok.d_nslow.p + 1, stream));
    HIP_OK(hipMemcpyAsync(b->tok.h_bad.p, b->tok.d_nslow.p, 2 * 4, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (b->tok.h_bad.p[1] || (n == 0 && nwords != 0)) return TM_EINVAL;
    if (n == 0) {   // no thread checked toff[0] == nwords == 0
        uint32_t t0 = 0;
        HIP_OK(hipMemcpy(&t0, b->tok.d_toff.p, 4, hipMemcpyDeviceToHost));
        if (t0 != 0) return TM_EINVAL;
    }
    b->dev_slow = true;
    return reserve_outputs(b);
}

int tm_engine::part_buffers(tm_batch* b, uint32_t n, uint64_t nwords, PartBuffers* out) {
    if (nwords > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    int rc;
    b->n = n;
    b->nwords = nwords;
    b->tokens_only = true;
    b->dev_tok = false;
    b->check_tokens = true;
    b->gbad = true;   // launched directly: the token check belongs to every launch
    b->launched = b->done = false;
    b->bytes.clear(); b->offs.clear();
    b->h_words.clear(); b->h_toff.clear(); b->h_tflags.clear(); b->h_slow.clear();
    if ((rc = b->tok.d_words.reserve(std::max<uint64_t>(nwords, 1)))) return rc;
    if ((rc = b->tok.d_toff.reserve((size_t)n + 1))) return rc;
    if ((rc = b->tok.d_tflags.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_slow.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_nslow.reserve(2))) return rc;
    if ((rc = b->tok.h_bad.reserve(2))) return rc;
    b->tok.h_bad.p[0] = b->tok.h_bad.p[1] = 0;
    b->dev_slow = true;
    if ((rc = reserve_outputs(b))) return rc;
    out->words = b->tok.d_words.p;
    out->toff = b->tok.d_toff.p;
    out->tflags = b->tok.d_tflags.p;
    out->words_cap = b->tok.d_words.cap;
    out->stream = st(b);
    out->device = b->rep->device;
    return TM_OK;
}

int tm_engine::export_batch(tm_batch* b, uint32_t* d_counts, uint32_t* d_ids, uint32_t mul, uint32_t add) {
    if (!b->done) return TM_EINVAL;
    if (int rc = ensure_dense(b)) return rc;
    const uint64_t top = (uint64_t)(nd.size() ? nd.size() - 1 : 0) * mul + add;
    if (top > 0xFFFFFFFFull) return TM_EOVERFLOW;
    HIP_OK(launch_export(b->dcsr.d_rowoff.p, b->dcsr.d_ids.p, b->n, b->total, d_counts, d_ids, mul, add, st(b)));
    HIP_OK(hipStreamSynchronize(st(b)));
    return TM_OK;
}

int tm_engine::reserve_hdr(tm_batch* b, size_t cap) {
    if (b->walk.d_hdr.p && b->walk.hdr_cap >= cap) return TM_OK;
    cap = std::max<size_t>(cap + cap / 4, 1024);
    DevBuf<uint8_t> nd;   // both new blocks first, then the old ones go
    PinBuf<uint8_t> nh;
    if (int rc = nd.alloc(tm_batch::hdr_bytes(cap))) return rc;
    if (nh.alloc(tm_batch::hdr_bytes(cap))) {
        snprintf(last_error(), 512, "hipHostMalloc of %zu bytes failed", tm_batch::hdr_bytes(cap));
        return TM_ENOMEM;
    }
    b->walk.d_hdr = std::move(nd);
    b->walk.h_hdr = std::move(nh);
    uint8_t *d = b->walk.d_hdr.p, *h = b->walk.h_hdr.p;
    b->walk.hdr_cap = cap;
    const size_t o_stats = CTRL_WORDS * 4, o_src = tm_batch::HDR_FIXED, o_count = o_src + cap * 8;
    b->walk.d_ctrl = (uint32_t*)d; b->walk.h_ctrl = (uint32_t*)h;
    b->walk.d_stats = (unsigned long long*)(d + o_stats); b->walk.h_stats = (unsigned long long*)(h + o_stats);
    b->walk.d_src = (unsigned long long*)(d + o_src); b->walk.h_src = (unsigned long long*)(h + o_src);
    b->walk.d_count = (uint32_t*)(d + o_count); b->walk.h_count = (uint32_t*)(h + o_count);
    return TM_OK;
}

int tm_engine::reserve_outputs(tm_batch* b) {
    int rc;
    const uint32_t n = b->n;
    const size_t nn = std::max<size_t>(n, 1);
    if ((rc = reserve_hdr(b, nn))) return rc;
    if ((rc = b->dcsr.d_rowoff.reserve(nn + 1))) return rc;
    if ((rc = b->dcsr.d_bsums.reserve((size_t)scan_block_count(n) + 1))) return rc;
    if ((rc = b->dcsr.d_ovf.reserve(nn))) return rc;
    if ((rc = b->dcsr.d_total.reserve(1))) return rc;
    if ((rc = reserve_rows(b))) return rc;
    if (!b->walk.ev0.e) {
        if ((rc = b->walk.ev0.create())) return rc;
        if ((rc = b->walk.ev1.create())) return rc;
        if ((rc = b->walk.ev2.create())) return rc;
        if ((rc = b->tok.evt.create())) return rc;
        if ((rc = b->dcsr.evc0.create())) return rc;
        if ((rc = b->dcsr.evc1.create())) return rc;
        if ((rc = b->walk.ev_end.create(hipEventDisableTiming))) return rc;
        if ((rc = b->walk.evq.create())) return rc;
    }
    return TM_OK;
}

int tm_engine::reserve_rows(tm_batch* b) {
    int rc;
    const uint64_t fast =
        std::max<uint64_t>((uint64_t)match_waves(b->n, b->rep->device, qcap) * tile_topics(b->n) * row_cap, 1);
    // + a byte per entry past the rows: the emission-log variant's lanes (TM_EMIT_LOG)
    if ((rc = b->walk.d_rows.reserve(fast + fast / 8 + 8))) return rc;
    if ((rc = b->walk.d_sfids.reserve(std::max<uint64_t>((uint64_t)b->n * 32, staging_min)))) return rc;
    if ((rc = b->dcsr.d_ids.reserve(std::max<uint64_t>((uint64_t)b->n * 32, 1u << 16)))) return rc;
    if ((rc = b->dcsr.h_total.reserve(4))) return rc;
    return TM_OK;
}

void tm_engine::dedup_topics(tm_batch* b, const uint8_t* topics, const uint64_t* offsets, uint32_t n) {
    std::vector<uint64_t> h(n);
    const unsigned nt = (n >= 65536) ? threads : 1;
    auto hash_range = [&](uint32_t lo, uint32_t hi) {
        for (uint32_t t = lo; t < hi; ++t) h[t] = hash_bytes(topics + offsets[t], offsets[t + 1] - offsets[t]);
    };
    if (nt <= 1) hash_range(0, n);
    else {
        std::vector<std::thread> th;
        for (unsigned i = 0; i < nt; ++i)
            th.emplace_back(hash_range, (uint32_t)((uint64_t)n * i / nt), (uint32_t)((uint64_t)n * (i + 1) / nt));
        for (auto& x : th) x.join();
    }
    size_t cap = 1024;
    while (cap < (size_t)n * 2) cap <<= 1;
    std::vector<uint32_t> tab(cap, 0);          // distinct index + 1
    std::vector<uint32_t> first;                 // publish index of each distinct topic
    b->row_of.resize(n);
    for (uint32_t t = 0; t < n; ++t) {
        const uint8_t* p = topics + offsets[t];
        const size_t len = offsets[t + 1] - offsets[t];
        size_t i = h[t] & (cap - 1);
        for (;;) {
            const uint32_t u = tab[i];
            if (u == 0) {
                first.push_back(t);
                tab[i] = (uint32_t)first.size();
                b->row_of[t] = (uint32_t)first.size() - 1;
                break;
            }
            const uint32_t f = first[u - 1];
            const size_t fl = offsets[f + 1] - offsets[f];
            if (h[f] == h[t] && fl == len && memcmp(topics + offsets[f], p, len) == 0) {
                b->row_of[t] = u - 1;
                break;
            }
            i = (i + 1) & (cap - 1);
        }
    }
    const uint32_t nu = (uint32_t)first.size();
    b->offs.assign((size_t)nu + 1, 0);
    uint64_t tot = 0;
    for (uint32_t u = 0; u < nu; ++u) tot += offsets[first[u] + 1] - offsets[first[u]];
    b->bytes.resize(tot);
    uint64_t o = 0;
    for (uint32_t u = 0; u < nu; ++u) {
        const uint32_t f = first[u];
        const size_t len = offsets[f + 1] - offsets[f];
        if (len) memcpy(b->bytes.data() + o, topics + offsets[f], len);
        o += len;
        b->offs[u + 1] = o;
    }
    b->n = nu;
}

int tm_engine::prepare(tm_batch* b, const uint8_t* topics, const uint64_t* offsets, uint32_t n, uint32_t flags) {
    if (int rc = check_topics(offsets, n)) return rc;
    forget_launch(b);   // its previous results are gone
    b->dedup = (flags & TM_BATCH_DEDUP) != 0;
    b->n_pub = n;
    b->row_of.clear();
    b->dev_tok = false;
    b->dedup_dev = b->dedup_stale = b->rowof_host = false;
    if (device >= 0 && dev_tok) {
        b->launched = b->done = false;
        b->tokens_only = false;
        b->n = n;
        b->bytes.clear();
        b->offs.clear();
        int rc = upload_bytes(b, topics, offsets, n);
        if (rc || !b->dedup) return rc;
        // deduplicated on the device at launch, ahead of the tokeniser
        b->dedup_dev = b->dedup_stale = true;
        return reserve_dedup(b, offsets[n] - offsets[0]);
    }
    if (b->dedup) {
        dedup_topics(b, topics, offsets, n);
    } else {
        b->n = n;
        b->offs.assign(offsets, offsets + (size_t)n + 1);
        const uint64_t base = offsets[0];
        for (auto& o : b->offs) o -= base;
        b->bytes.assign(topics + base, topics + base + b->offs[n]);
    }
    b->launched = b->done = false;
    b->tokens_only = false;
    int rc = tokenize(b);
    if (rc) return rc;
    if (device < 0) return TM_OK;
    return upload_batch(b);
}

void tm_engine::drop_user_stream(tm_batch* b) {
    auto& rd = b->rep->readers;
    rd.erase(std::remove(rd.begin(), rd.end(), b), rd.end());
    if (b->own) (void)hipStreamDestroy(b->own);
    b->own = nullptr;
    b->own_user = false;
}

int tm_engine::upload_bytes(tm_batch* b, const uint8_t* topics, const uint64_t* offsets, uint32_t n) {
    int rc;
    const hipStream_t S = st(b);
    const uint64_t base = offsets[0], nbytes = offsets[n] - base;
    if (nbytes + n + 1 > 0xFFFFFFF0ull) return TM_EOVERFLOW;   // u32 word offsets
    b->tok_base = base;
    if ((rc = b->tok.d_bytes.reserve(nbytes + 16))) return rc;   // +16: no tail reads past
    if ((rc = b->tok.d_boffs.reserve((size_t)n + 1))) return rc;
    if ((rc = reserve_tokens(b, n, nbytes))) return rc;
    if (nbytes) HIP_OK(hipMemcpyAsync(b->tok.d_bytes.p, topics + base, nbytes, hipMemcpyHostToDevice, S));
    HIP_OK(hipMemcpyAsync(b->tok.d_boffs.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, S));
    // the caller's buffers are only borrowed for the call; tm_match_batch
    // (and the async slots, whose inputs are their own pinned buffers)
    // wait for the whole pipeline later, so they skip this sync
    if (!upload_nosync && !b->own) HIP_OK(hipStreamSynchronize(S));
    b->tok.in_bytes = b->tok.d_bytes.p;
    b->tok.in_offs = b->tok.d_boffs.p;
    return tokens_pending(b);
}

int tm_engine::reserve_tokens(tm_batch* b, uint32_t n, uint64_t nbytes) {
    int rc;
    b->nwords = nbytes + n;                  // bound: one word per byte + 1 per topic
    if ((rc = b->tok.d_wcount.reserve((size_t)n + 2))) return rc;   // per tile + total
    if ((rc = b->tok.d_words.reserve(std::max<uint64_t>(b->nwords, 1)))) return rc;
    if ((rc = b->tok.d_toff.reserve((size_t)n + 1))) return rc;
    if ((rc = b->tok.d_tflags.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_slow.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->tok.d_nslow.reserve(2))) return rc;
    return TM_OK;
}

int tm_engine::reserve_dedup(tm_batch* b, uint64_t nbytes) {
    int rc;
    const size_t n = b->n;
    if (nbytes >> DD_OFF_BITS) {   // (a table slot holds a 40-bit byte offset)
        snprintf(last_error(), 512, "device dedup: batch of %llu bytes over 2^40", (unsigned long long)nbytes);
        return TM_EINVAL;
    }
    uint64_t cap = 1024;
    while (cap < (uint64_t)n + n / 2) cap <<= 1;   // load <= 2/3 when every publish is distinct
    const uint64_t old_mask = b->dtab_mask;
    b->dtab_mask = cap - 1;
    b->dd_bytes = nbytes;
    const size_t nblk = dedup_blocks((uint32_t)n);
    const size_t nb = scan_block_count((uint32_t)nblk) + 1;
    void* old_tab = b->dd.d_dtab.p;
    if ((rc = b->dd.d_dtab.reserve(cap))) return rc;
    if (b->dd.d_dtab.p != old_tab || old_mask != b->dtab_mask) b->dtab_dirty = true;
    if ((rc = b->dd.d_dsrow.reserve(cap))) return rc;
    if ((rc = b->dd.d_dsmeta.reserve(cap))) return rc;
    if ((rc = b->dd.d_drrep.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->dd.d_dbsum.reserve(n / DD_EXPAND_TILE + 2))) return rc;   // (expansion blocks)
    if ((rc = b->dd.d_dslot.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->dd.d_dbits.reserve(std::max<size_t>(nblk, 1) * (DD_TILE / 64)))) return rc;
    if ((rc = b->dd.d_dbc.reserve(nblk + 1))) return rc;
    if ((rc = b->dd.d_dbb.reserve(nblk + 1))) return rc;
    if ((rc = b->dd.d_drbs.reserve(nb))) return rc;
    if ((rc = b->dd.d_dbbs.reserve(nb))) return rc;
    if ((rc = b->dd.d_rowof.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->dd.d_cbytes.reserve(nbytes + 32))) return rc;   // (the tokeniser's 16-B windows)
    if ((rc = b->dd.d_coffs.reserve(n + 1))) return rc;
    if ((rc = b->dd.d_dd.reserve(2))) return rc;
    if ((rc = b->dd.d_pcount.reserve(std::max<size_t>(n, 1)))) return rc;
    if ((rc = b->dd.d_psrc.reserve(std::max<size_t>(n, 1)))) return rc;
    if (!b->dd.evd.e) {
        if ((rc = b->dd.evd.create())) return rc;
        if ((rc = b->dd.evx0.create())) return rc;
        if ((rc = b->dd.evx1.create())) return rc;
    }
    return TM_OK;
}

DedupArgs tm_engine::dedup_args(tm_batch* b) const {
    DedupArgs d{};
    d.bytes = b->tok.in_bytes; d.offs = b->tok.in_offs; d.base = b->tok_base; d.n = b->n_pub;
    d.table = b->dd.d_dtab.p; d.mask = b->dtab_mask;
    d.slot = b->dd.d_dslot.p; d.repbits = b->dd.d_dbits.p; d.bcount = b->dd.d_dbc.p; d.bbytes = b->dd.d_dbb.p;
    d.rbs = b->dd.d_drbs.p; d.bbs = b->dd.d_dbbs.p; d.srow = b->dd.d_dsrow.p; d.rrep = b->dd.d_drrep.p;
    d.smeta = b->dd.d_dsmeta.p;
    d.row_of = b->dd.d_rowof.p; d.cbytes = b->dd.d_cbytes.p; d.coffs = b->dd.d_coffs.p; d.dd = b->dd.d_dd.p;
    d.ctrl = b->walk.d_ctrl; d.count = b->walk.d_count; d.src = b->walk.d_src;
    d.pcount = b->dd.d_pcount.p; d.psrc = b->dd.d_psrc.p;
    d.stats = b->walk.d_stats;
    d.bsum = b->dd.d_dbsum.p;
    d.weak_hash = kn.dedup_weak_hash ? 1u : 0u;
    return d;
}

// the dedup passes (no table clear: clear_dedup_table, outside any capture)
int tm_engine::enqueue_dedup(tm_batch* b, hipStream_t S) {
    const DedupArgs d = dedup_args(b);
    if (!d.n) HIP_OK(hipMemsetAsync(b->dd.d_dd.p, 0, 8, S));   // (no compact kernel: zero rows)
    const uint32_t nblk = dedup_blocks(d.n);
    ScanArgs rs{}, bs{};
    rs.count = d.bcount; rs.row_off = d.bcount; rs.block_sums = b->dd.d_drbs.p; rs.n = nblk;   // (in place)
    bs.count = d.bbytes; bs.row_off = d.bbytes; bs.block_sums = b->dd.d_dbbs.p; bs.n = nblk;
    HIP_OK(launch_dedup(d, rs, bs, S));
    return TM_OK;
}

// a dirty table (new, or a pass whose expansion was not waited for) is
// cleared before the next pass; a clean one is zero already
int tm_engine::clear_dedup_table(tm_batch* b, hipStream_t S) {
    if (b->dtab_dirty) HIP_OK(hipMemsetAsync(b->dd.d_dtab.p, 0, (b->dtab_mask + 1) * 8, S));
    b->dtab_dirty = true;   // until this pass's expansion has been waited for
    return TM_OK;
}

int tm_engine::tokens_pending(tm_batch* b) {
    b->h_words.clear(); b->h_toff.clear(); b->h_tflags.clear(); b->h_slow.clear();
    b->dev_tok = true;
    b->tok_dict = ~0ull;
    b->dev_slow = true;
    return reserve_outputs(b);
}

int tm_engine::upload_packed(tm_batch* b, const uint8_t* blk, uint32_t n, uint64_t nbytes) {
    int rc;
    const size_t head = packed_head(n);
    if (nbytes + n + 1 > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    b->dedup = false;
    b->bounded = false;
    b->n_pub = n;
    b->row_of.clear();
    b->launched = b->done = false;
    b->tokens_only = false;
    b->n = n;
    b->bytes.clear();
    b->offs.clear();
    b->tok_base = 0;
    if ((rc = reserve_tokens(b, n, nbytes))) return rc;
    if ((rc = b->tok.d_in.reserve(head + nbytes + 16))) return rc;   // +16: no tail reads past
    HIP_OK(hipMemcpyAsync(b->tok.d_in.p, blk, head + nbytes, hipMemcpyHostToDevice, b->own));
    b->tok.in_offs = reinterpret_cast<const uint64_t*>(b->tok.d_in.p);
    b->tok.in_bytes = b->tok.d_in.p + head;
    return tokens_pending(b);
}

// An async slot's bounded batch (see tm_batch::bounded): sized for `bound`
// topics and `bytes_cap` bytes; its offsets, bytes and count live in mapped
// pinned memory (d_offs / d_bytes / d_n, device pointers), written by the
// slot before every launch.  Called before every launch (cheap once sized):
// the tokens are made fresh each time.
int tm_engine::prepare_bounded(tm_batch* b, uint32_t bound, uint64_t bytes_cap, const uint64_t* d_offs,
                               const uint8_t* d_bytes, uint32_t* d_n) {
    int rc;
    if (bytes_cap + bound + 1 > 0xFFFFFFF0ull) return TM_EOVERFLOW;
    b->dedup = b->dedup_dev = false;
    b->n_pub = bound;
    b->n = bound;
    b->row_of.clear();
    b->launched = b->done = false;
    b->tokens_only = false;
    b->bytes.clear();
    b->offs.clear();
    b->tok_base = 0;
    if ((rc = reserve_tokens(b, bound, bytes_cap))) return rc;
    b->tok.in_offs = d_offs;
    b->tok.in_bytes = d_bytes;
    b->d_nb = d_n;
    b->bounded = true;
    return tokens_pending(b);
}

// A captured deduplicated batch replayed: its timing events are recorded on
// the stream around the graph (an event record inside that capture is refused
// by the runtime), so the replay's whole span is its walk time.
hipError_t tm_engine::graph_replay(tm_batch* b, hipStream_t S) {
    hipError_t e;
    if (b->dedup_timed && (e = hipEventRecord(b->dd.evd.e, S)) != hipSuccess) return e;
    if ((e = hipEventRecord(b->walk.ev0.e, S)) != hipSuccess) return e;
    if ((e = hipGraphLaunch(b->graph.exec, S)) != hipSuccess) return e;
    if ((e = hipEventRecord(b->walk.ev1.e, S)) != hipSuccess) return e;
    if ((e = hipEventRecord(b->walk.ev2.e, S)) != hipSuccess) return e;
    ++graph_launches;
    return hipSuccess;
}

// (the policy: tm_engine_impl.hpp)
template <class Record>
bool tm_engine::graph_ready(GraphCache& gc, bool& gbad, std::vector<uint8_t>& key, hipStream_t S, Record&& record) {
    if (gc.exec && gc.key == key) return true;
    if (gc.exec) (void)hipGraphExecDestroy(gc.exec);
    gc.exec = nullptr;
    if (gc.key == key) {   // the second launch with these arguments: capture them
        hipGraph_t g = nullptr;
        if (hipStreamBeginCapture(S, hipStreamCaptureModeRelaxed) == hipSuccess) {
            const hipError_t e = record();
            const hipError_t e2 = hipStreamEndCapture(S, &g);
            if (e != hipSuccess || e2 != hipSuccess || !g ||
                hipGraphInstantiate(&gc.exec, g, nullptr, nullptr, 0) != hipSuccess)
                gc.exec = nullptr;
            if (g) (void)hipGraphDestroy(g);
        }
        if (!gc.exec) {
            (void)hipGetLastError();
            gbad = true;   // the direct way from now on
        }
    }
    gc.key.swap(key);
    return gc.exec != nullptr;
}

int tm_engine::launch(tm_batch* b, bool csr, SlotTail* tail) {
    if (reps.empty()) return TM_ENODEV;
    int rc;
    Replica& R = *b->rep;
    const hipStream_t S = st(b);
    if (!b->tokens_only && !b->dev_tok && b->dict_size != dict.size()) {   // new words since tokenisation
        if ((rc = tokenize(b))) return rc;
        if ((rc = upload_batch(b))) return rc;
    }
    if (csr) HIP_OK(hipEventRecord(b->walk.evq.e, S));   // (before the delta upload and the waits below)
    if ((rc = sync_device(&R))) return rc;
    if (b->own && b->seen_upload != R.upload_seq) {   // trie deltas still in flight on the replica stream land first
        HIP_OK(hipStreamWaitEvent(S, R.tab.ev_sync.e, 0));
        b->seen_upload = R.upload_seq;
    }
    if ((rc = ensure_slow_scratch(b))) return rc;
    if (checked) {
        if ((rc = R.tab.d_dbg.reserve(8))) return rc;
        if ((rc = R.tab.h_dbg.reserve(8))) return rc;
        HIP_OK(hipMemsetAsync(R.tab.d_dbg.p, 0, 8 * 4, S));
    }
    // A device-deduplicated batch: fresh bytes are deduplicated first, and
    // only the rows are tokenised (again when the dictionary grew) and
    // walked.  The rows are counted on the device, so the tokeniser and
    // the walk are sized for every publish (the bound) and read the count
    // there; wait() sets n to the rows.
    const bool dedup_now = b->dedup_dev && b->dedup_stale;
    const bool tokenize_now = b->dev_tok && (b->tok_dict != dict.size() || dedup_now);
    if (b->dedup_dev) b->n = b->n_pub;
    b->dedup_timed = dedup_now && csr;
    const bool graph = csr && !checked && !tokenize_now && use_graphs && !b->gbad && b->n <= GRAPH_MAX &&
                       !b->dedup_dev;
    // a fresh device-deduplicated batch (C5: every launch) replays its whole
    // sequence -- dedup, tokeniser, walk, expand, read-back -- as one captured
    // graph: ~25 enqueues cost ~0.2 ms of host time per launch otherwise
    const bool dgraph = csr && !checked && use_graphs && !b->gbad && b->dedup_dev && dedup_now && tokenize_now &&
                        !b->check_tokens;
    b->tok_timed = tokenize_now && csr;
    TokArgs t{};
    ScanArgs ts{};
    if (tokenize_now) {
        b->tok_dict = dict.size();
        t.zero = reinterpret_cast<uint32_t*>(b->walk.d_hdr.p);   // the tokeniser's first kernel clears ctrl + stats
        t.zero_words = tm_batch::HDR_FIXED / 4;
        t.bytes = b->tok.in_bytes; t.offs = b->tok.in_offs; t.base = b->tok_base; t.n = b->n;
        t.keys = R.tab.d_dkey.p; t.tails = R.tab.d_tail.p; t.dict_mask = R.d_dict_n - 1; t.arena = R.tab.d_arena.p;
        t.wcount = b->tok.d_wcount.p; t.tflags = b->tok.d_tflags.p;
        t.toff = b->tok.d_toff.p; t.words = b->tok.d_words.p;
        t.words_cap = b->tok.d_words.cap;
        t.slow_list = b->tok.d_slow.p; t.d_nslow = b->tok.d_nslow.p;
        t.tile_topics = tok_tile_topics(b->n, b->nwords - b->n);   // nwords = bytes + topics (reserve_tokens)
        t.d_n = nullptr;
        if (b->dedup_dev) {   // the rows' bytes, compacted by the dedup pass
            t.bytes = b->dd.d_cbytes.p; t.offs = b->dd.d_coffs.p; t.base = 0; t.d_n = b->dd.d_dd.p;
        }
        if (b->bounded) t.d_n = b->d_nb;   // (sized for the bound, counted in pinned memory)
        ts.block_sums = b->dcsr.d_bsums.p;
    }
    MatchArgs a{};
    a.slots = R.tab.d_slots.p;
    a.nbuckets = nbuckets();
    // (a bound on the probe run, not the exact max_disp: a longer run stops
    // at its first bucket with a free last slot all the same, and a value
    // that changes only at these steps keeps the captured launch graphs of
    // churned batches valid)
    // Every insert path bounds max_disp by MAX_PROBE_DISP before it returns; a
    // table it could not bring under the bound is not launched against, and
    // the clamp keeps the kernel argument inside the walk's displacement field
    // whatever the host believes.
    if (max_disp > MAX_PROBE_DISP) return probe_bound_error();
    static_assert(MAX_PROBE_DISP >= 16, "the steps below end at the bound");
    a.max_probe = max_disp <= 4 ? 4 : max_disp <= 8 ? 8 : max_disp <= 16 ? 16 : MAX_PROBE_DISP;
    a.root = root_rec();
    a.foff = R.tab.d_foff.p; a.flen = R.tab.d_flen.p; a.fbytes = R.tab.d_fbytes.p;
    a.words = b->tok.d_words.p; a.toff = b->tok.d_toff.p; a.tflags = b->tok.d_tflags.p; a.n = b->n;
    a.slow_list = b->tok.d_slow.p; a.n_slow = b->dev_slow ? 0u : (uint32_t)b->h_slow.size();
    a.d_nslow = b->dev_slow ? b->tok.d_nslow.p : nullptr;
    a.d_n = b->dedup_dev ? b->dd.d_dd.p : b->bounded ? b->d_nb : nullptr;   // the rows, counted by the dedup pass
    a.count = b->walk.d_count; a.src = b->walk.d_src; a.rows = b->walk.d_rows.p; a.row_cap = row_cap;
    a.grid = match_waves(b->n, R.device, qcap);
    a.tile_topics = tile_topics(b->n);
    a.qcap = qcap;
    {   // the first static_frac of the tiles round-robin, the tail by per-XCD tickets
        const uint64_t ntiles = ((uint64_t)b->n + a.tile_topics - 1) / a.tile_topics;
        a.static_rounds = std::max<uint32_t>(1, (uint32_t)(static_frac * (double)ntiles / std::max(a.grid, 1u)));
    }
    if ((uint64_t)a.grid * a.tile_topics * row_cap > b->walk.d_rows.cap) {
        snprintf(last_error(), 512, "emission rows sized for fewer waves than the launch");
        return TM_EIO;
    }
    a.sfids = b->walk.d_sfids.p; a.sfids_cap = std::min<uint64_t>(b->walk.d_sfids.cap, MAX_RESULT);
    a.rcap = region_cap(a.sfids_cap, b->one_region);
    a.sgmask = b->one_region ? 0u : TICKET_GROUPS - 1;
    a.xg = b->walk.d_ctrl + XG_WORD;
    a.ctrl = b->walk.d_ctrl; a.ovf_list = b->dcsr.d_ovf.p;
    a.ovf_cap = (uint32_t)std::min<size_t>(b->dcsr.d_ovf.cap, 0xFFFFFFF0ull);
    a.stats = b->walk.d_stats;
    // a walk of many waves writes per-wave sums (one reduce kernel after it);
    // a small one adds them atomically -- a few dozen same-line atomics cost
    // less than one more launch on the per-publish path
    if (a.grid >= WSTATS_MIN_WAVES) {
        if ((rc = b->walk.d_wstats.reserve((size_t)a.grid * WSTATS))) return rc;
        a.wstats = b->walk.d_wstats.p;
    }
    a.s_qparent = b->gen.d_sqpar.p; a.s_qpw = b->gen.d_sqpw.p;
    a.s_qmeta = b->gen.d_sqmeta.p; a.s_qkey = b->gen.d_sqkey.p;
    a.s_ofid = b->gen.d_sofid.p; a.s_okey = b->gen.d_sokey.p;
    a.s_qcap = b->s_qcap; a.s_ocap = b->s_ocap; a.s_waves = b->s_waves; a.s_lcap = kn.slow_lds;
    a.nwords = (uint32_t)std::max<uint64_t>(b->nwords, 1);
    a.nslots = (uint32_t)slots.size();
    // (bounds of the checked build only: left 0 otherwise, so churn does not
    // change the launch's arguments and a captured graph stays valid)
    a.nnodes = checked ? (uint32_t)nd.size() : 0u;
    a.nfbytes = checked ? fbytes.size() : 0u;
    a.dbg = checked ? R.tab.d_dbg.p : nullptr;
    ScanArgs s{};
    s.count = b->walk.d_count; s.src = b->walk.d_src;
    s.sfids = b->walk.d_sfids.p; s.sfids_cap = std::min<uint64_t>(b->walk.d_sfids.cap, MAX_RESULT);
    s.row_off = b->dcsr.d_rowoff.p; s.ids = b->dcsr.d_ids.p; s.block_sums = b->dcsr.d_bsums.p;
    s.n = b->n; s.ids_cap = (uint32_t)std::min<size_t>(b->dcsr.d_ids.cap, 0xFFFFFFF0ull); s.ctrl = b->walk.d_ctrl;
    s.dbg = checked ? R.tab.d_dbg.p : nullptr;
    b->end_recorded = false;
    b->graphed = false;
    b->dense_enq = false;
    // Everything the launch puts on the stream (cap: captured into a graph,
    // without the timing events -- the runtime refuses event records inside this
    // capture, so graph_replay records them around the whole graph; csr_too:
    // the read-back of ctrl + stats as well)
    auto enqueue = [&](bool cap, bool csr_too) -> hipError_t {
        hipError_t e;
        if (!tokenize_now && (e = hipMemsetAsync(b->walk.d_hdr.p, 0, tm_batch::HDR_FIXED, S)) != hipSuccess) return e;
        if (dedup_now) {
            if (b->dedup_timed && !cap && (e = hipEventRecord(b->dd.evd.e, S)) != hipSuccess) return e;
            if (enqueue_dedup(b, S) != TM_OK) return hipErrorUnknown;
        }
        if (b->tok_timed && !cap && (e = hipEventRecord(b->tok.evt.e, S)) != hipSuccess) return e;
        if (tokenize_now && (e = launch_tokenize(t, ts, b->tok.d_nslow.p + 1, S)) != hipSuccess) return e;
        if (b->check_tokens && b->n) {
            if ((e = hipMemsetAsync(b->tok.d_nslow.p, 0, 2 * 4, S)) != hipSuccess) return e;
            if ((e = launch_token_check(b->tok.d_toff.p, b->tok.d_tflags.p, b->n, b->nwords, b->tok.d_slow.p,
                                        b->tok.d_nslow.p, b->tok.d_nslow.p + 1, S)) != hipSuccess)
                return e;
        }
        e = launch_match(a, S, csr && !cap ? b->walk.ev0.e : nullptr, csr && !cap ? b->walk.ev1.e : nullptr, checked,
                         0u);
        if (e != hipSuccess) return e;
        if (b->dedup_dev) {   // every publish's row (count, start) + the delivered matches
            if (!cap && (e = hipEventRecord(b->dd.evx0.e, S)) != hipSuccess) return e;
            if ((e = launch_dedup_expand(dedup_args(b), S)) != hipSuccess) return e;
            if (!cap && (e = hipEventRecord(b->dd.evx1.e, S)) != hipSuccess) return e;
        }
        if (cap && csr_too)   // (ev2 is recorded after the graph's launch)
            return hipMemcpyAsync(b->walk.h_hdr.p, b->walk.d_hdr.p, tm_batch::HDR_FIXED, hipMemcpyDeviceToHost, S);
        return csr_too ? enqueue_csr(b, S) : hipSuccess;
    };
    // At most one of the three captured forms applies (graph_ready decides
    // replay, capture or direct); grc 0: a graph holds the launch, 1: direct
    int grc = 1;
    if (graph) {   // a repeated tokenised batch: memset + walk + read-back replayed
        std::vector<uint8_t> key = graph_key({}, a, s);
        auto record = [&] {
            hipError_t e = hipMemsetAsync(b->walk.d_hdr.p, 0, tm_batch::HDR_FIXED, S);
            // timing events as external nodes: every replay re-records them
            if (e == hipSuccess) e = launch_match(a, S, b->walk.ev0.e, b->walk.ev1.e, false, hipEventRecordExternal);
            if (e == hipSuccess) e = enqueue_csr(b, S, hipEventRecordExternal);
            return e;
        };
        if (graph_ready(b->graph, b->gbad, key, S, record)) {
            HIP_OK(hipGraphLaunch(b->graph.exec, S));
            ++graph_launches;
            grc = 0;
        }
    }
    bool csr_done = false;
    if (dedup_now && (rc = clear_dedup_table(b, S))) return rc;   // (outside the capture below)
    if (dgraph) {
        const DedupArgs d = dedup_args(b);
        std::vector<uint8_t> key = graph_key({}, t, ts, a, s, d);
        const std::vector<uint8_t>& old = b->graph.key;
        if (kn.par_trace && !(b->graph.exec && old == key) && old.size() == key.size()) {
            // which arguments changed (offsets per struct)
            const size_t ends[5] = {sizeof t, sizeof t + sizeof ts, sizeof t + sizeof ts + sizeof a,
                                    sizeof t + sizeof ts + sizeof a + sizeof s, key.size()};
            const char* names[5] = {"tok", "tscan", "match", "scan", "dedup"};
            fprintf(stderr, "[graph key miss]");
            size_t st = 0;
            for (int q = 0; q < 5; ++q) {
                for (size_t i = st; i < ends[q]; i += 4)
                    if (memcmp(&key[i], &old[i], std::min<size_t>(4, ends[q] - i)))
                        fprintf(stderr, " %s+%zu", names[q], i - st);
                st = ends[q];
            }
            fprintf(stderr, "\n");
        }
        if (graph_ready(b->graph, b->gbad, key, S, [&] { return enqueue(true, true); })) {
            HIP_OK(graph_replay(b, S));
            grc = 0;
        }
        csr_done = grc == 0;
        if (csr_done) { b->tok_timed = false; b->graphed = true; }   // (replayed: see the enqueue above)
    }
    // A bounded batch (an async slot's): the same arguments every launch, so
    // from its second launch on the tokeniser, the walk, the generic path and
    // the slot's tail (export + flag) replay as one captured graph: ~10
    // enqueues of ~3 us host time each become one
    if (tail && !csr && b->bounded && tokenize_now && use_graphs && !checked && !b->gbad && grc == 1) {
        std::vector<uint8_t> key = graph_key(tail->key, t, ts, a, s);
        auto record = [&] {
            const hipError_t e = enqueue(true, false);
            return e == hipSuccess ? tail->run(S) : e;
        };
        if (graph_ready(tail->gc, b->gbad, key, S, record)) {
            HIP_OK(hipGraphLaunch(tail->gc.exec, S));
            ++graph_launches;
            grc = 0;
        }
        tail->in_graph = grc == 0;
    }
    if (grc == 1) {
        const hipError_t e = enqueue(false, false);
        if (e != hipSuccess) {
            snprintf(last_error(), 512, "%s at launch (%s)", hipGetErrorString(e), __FILE_NAME__);
            return TM_EIO;
        }
    }
    if (dedup_now) {   // (enqueued: a failed launch dedups again next time)
        b->dedup_stale = false;
        b->rowof_host = false;
    }
    note_launch(b);
    b->launched = true;
    b->done = false;
    b->dense = false;
    b->csr = csr;
    if (!csr) return TM_OK;   // the async slot enqueues its read-back and event
    if (grc == 1 && !csr_done) HIP_OK(enqueue_csr(b, S));   // (a graph holds it)
    b->scan_args = s;
    if (b->check_tokens) HIP_OK(hipMemcpyAsync(b->tok.h_bad.p, b->tok.d_nslow.p, 2 * 4, hipMemcpyDeviceToHost, S));
    if (checked) HIP_OK(hipMemcpyAsync(R.tab.h_dbg.p, R.tab.d_dbg.p, 8 * 4, hipMemcpyDeviceToHost, S));
    if (b->oneshot || b->eager_dense) {
        if ((rc = enqueue_dense_tail(b, S))) return rc;
        b->dense_enq = true;
    }
    HIP_OK(hipEventRecord(b->walk.ev_end.e, S));
    b->end_recorded = true;
    return TM_OK;
}

hipError_t tm_engine::enqueue_csr(tm_batch* b, hipStream_t S, unsigned ev_flags) {
    hipError_t e;
    if ((e = hipEventRecordWithFlags(b->walk.ev2.e, S, ev_flags)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(b->walk.h_hdr.p, b->walk.d_hdr.p, tm_batch::HDR_FIXED, hipMemcpyDeviceToHost, S)) !=
        hipSuccess)
        return e;   // ctrl + stats
    return hipSuccess;
}

int tm_engine::enqueue_dense_tail(tm_batch* b, hipStream_t S) {
    int rc;
    ScanArgs s = b->scan_args;
    s.ids = b->dcsr.d_ids.p;
    s.ids_cap = (uint32_t)std::min<size_t>(b->dcsr.d_ids.cap, 0xFFFFFFF0ull);
    b->dense_cap = s.ids_cap;
    if (!b->oneshot) {   // the dense CSR only (the pipelined tm_match_batch copies it by DMA)
        HIP_OK(hipEventRecord(b->dcsr.evc0.e, S));
        HIP_OK(launch_scan(s, S, b->dcsr.d_total.p));
        HIP_OK(launch_finalize(s, S, false));
        HIP_OK(hipEventRecord(b->dcsr.evc1.e, S));
        return TM_OK;
    }
    if ((rc = b->dcsr.h_xrow.reserve(((size_t)b->n + 1) * 4))) return rc;
    if ((rc = b->dcsr.h_xids.reserve(std::max<size_t>(b->dcsr.d_ids.cap, 1) * 4))) return rc;
    void *d_row = nullptr, *d_ids = nullptr;
    HIP_OK(hipHostGetDevicePointer(&d_row, b->dcsr.h_xrow.p, 0));
    HIP_OK(hipHostGetDevicePointer(&d_ids, b->dcsr.h_xids.p, 0));
    b->x_cap = std::min<uint64_t>(s.ids_cap, b->dcsr.h_xids.cap / 4);
    HIP_OK(hipEventRecord(b->dcsr.evc0.e, S));
    HIP_OK(launch_scan(s, S, b->dcsr.d_total.p));
    HIP_OK(launch_finalize(s, S, false));
    HIP_OK(hipEventRecord(b->dcsr.evc1.e, S));
    HIP_OK(launch_csr_to_host(b->dcsr.d_rowoff.p, b->dcsr.d_ids.p, b->n, b->dcsr.d_total.p, b->x_cap,
                              static_cast<uint32_t*>(d_row), static_cast<uint32_t*>(d_ids), S));
    return TM_OK;
}

int tm_engine::oneshot_result(tm_batch* b, tm_result* out) {
    const uint32_t* row = reinterpret_cast<const uint32_t*>(b->dcsr.h_xrow.p);
    if (!b->oneshot || !b->done || b->total > b->x_cap || row[b->n] != b->total || row[0] != 0) return 1;
    float ms = 0;
    (void)hipEventElapsedTime(&ms, b->dcsr.evc0.e, b->dcsr.evc1.e);
    b->st.ms_csr = ms;
    b->dense = true;
    out->n_topics = b->n;
    out->n_matches = b->total;
    out->row_offsets = row;
    out->filter_ids = reinterpret_cast<const uint32_t*>(b->dcsr.h_xids.p);
    return TM_OK;
}

int tm_engine::ensure_dense(tm_batch* b) {
    if (!b->done) return TM_EINVAL;
    if (b->dense) return TM_OK;
    const hipStream_t S = st(b);
    int rc;
    if (b->total > b->dcsr.d_ids.cap) {
        if ((rc = b->dcsr.d_ids.reserve((size_t)b->total + b->total / 4))) return rc;
    }
    b->scan_args.ids = b->dcsr.d_ids.p;
    b->scan_args.ids_cap = (uint32_t)std::min<size_t>(b->dcsr.d_ids.cap, 0xFFFFFFF0ull);
    HIP_OK(hipEventRecord(b->dcsr.evc0.e, S));
    HIP_OK(launch_scan(b->scan_args, S, b->dcsr.d_total.p));
    HIP_OK(launch_finalize(b->scan_args, S, checked));
    HIP_OK(hipEventRecord(b->dcsr.evc1.e, S));
    HIP_OK(hipMemcpyAsync(b->dcsr.h_total.p, b->dcsr.d_total.p, 4, hipMemcpyDeviceToHost, S));
    HIP_OK(hipStreamSynchronize(S));
    if (b->dcsr.h_total.p[0] != b->total) {
        snprintf(last_error(), 512, "inconsistent CSR: scanned %u entries, kernel count %llu", b->dcsr.h_total.p[0],
                 (unsigned long long)b->total);
        return TM_EIO;
    }
    float ms = 0;
    (void)hipEventElapsedTime(&ms, b->dcsr.evc0.e, b->dcsr.evc1.e);
    b->st.ms_csr = ms;
    b->dense = true;
    return TM_OK;
}

int tm_engine::check_ctrl(const uint32_t* ctrl, const unsigned long long* stats, uint32_t* err, uint64_t* need,
               uint64_t* staged_out) {
    *err = ctrl[CTRL_ERR];
    uint64_t staged = 0, top = 0;
    for (uint32_t g = 0; g < TICKET_GROUPS; ++g) {
        const uint64_t t = xg_top_read(ctrl, g);
        staged += t;
        top = std::max(top, t);
    }
    *need = top * TICKET_GROUPS;   // staging capacity that holds every region's reservation
    if (staged_out) *staged_out = staged;
    const uint64_t nmatch = stats[ST_MATCHES];
    // a CSR with u32 offsets cannot hold more (tm_result): refuse, never wrap
    if ((*err & ERR_CSR_RANGE) || staged > result_limit || nmatch > result_limit) {
        snprintf(last_error(), 512, "batch result too large: %llu staged / %llu matched > limit %llu",
                 (unsigned long long)staged, (unsigned long long)nmatch, (unsigned long long)result_limit);
        return TM_EOVERFLOW;
    }
    return TM_OK;
}

int tm_engine::grow_for(tm_batch* b, uint32_t err, uint64_t need, uint64_t staged) {
    if (err & ERR_STAGING) {
        // per-group regions of the largest group's size: unless that exceeds
        // the limit while the batch as a whole fits (skew concentrated in one
        // walk group) -- then one region for all groups, sized by the total
        const uint64_t limit = std::min<uint64_t>(MAX_RESULT, result_limit + 1024);
        if (!b->one_region && need + need / 4 + 1024 > limit && staged <= result_limit) b->one_region = true;
        if (b->one_region) need = staged;
        int rc = b->walk.d_sfids.reserve(std::min<uint64_t>(need + need / 4 + 1024, limit));
        if (rc) return rc;
    }
    if (err & ERR_SLOW_SCRATCH) {
        b->s_qcap *= 4;
        b->s_ocap *= 4;
    }
    return TM_OK;
}

void tm_engine::fill_stats(tm_batch* b) {
    float ms_match = 0, ms_total = 0, ms_tok = 0, ms_dd = 0, ms_x = 0;
    (void)hipEventElapsedTime(&ms_match, b->walk.ev0.e, b->walk.ev1.e);
    (void)hipEventElapsedTime(&ms_total, b->walk.ev0.e, b->walk.ev2.e);
    if (b->tok_timed) (void)hipEventElapsedTime(&ms_tok, b->tok.evt.e, b->walk.ev0.e);
    if (b->dedup_timed) (void)hipEventElapsedTime(&ms_dd, b->dd.evd.e, b->tok_timed ? b->tok.evt.e : b->walk.ev0.e);
    if (b->dedup_dev && !b->graphed) (void)hipEventElapsedTime(&ms_x, b->dd.evx0.e, b->dd.evx1.e);
    b->st.ms_tokenize = ms_tok;
    b->st.ms_dedup = ms_dd;
    b->st.ms_expand = ms_x;
    b->st.publishes = b->dedup ? b->n_pub : b->n;
    float ms_q = 0;
    (void)hipEventElapsedTime(&ms_q, b->walk.evq.e,
                              b->dedup_timed ? b->dd.evd.e : b->tok_timed ? b->tok.evt.e : b->walk.ev0.e);
    b->st.ms_queue = ms_q;
    b->st.ms_csr = 0;   // set by ensure_dense
    b->st.topics = b->n;
    b->st.visits = b->walk.h_stats[ST_VISITS];
    b->st.hash_hits = b->walk.h_stats[ST_HASH];
    b->st.words = b->walk.h_stats[ST_WORDS];
    b->st.matches = b->walk.h_stats[ST_MATCHES];
    b->st.slow_topics = b->walk.h_stats[ST_SLOW];
    b->st.probes = b->walk.h_stats[ST_PROBES];
    b->st.iterations = b->walk.h_stats[ST_ITERS];
    b->st.overflow_tiles = b->walk.h_ctrl[CTRL_NOVF];
    b->st.ms_match = ms_match;
    b->st.ms_total = ms_total;
    b->total = b->st.matches;
    b->st.delivered = b->dedup_dev ? b->walk.h_stats[ST_DELIVERED] : b->st.matches;
#if TM_PHASE_CYCLES
    // dev build: the tile walk's cycle sums over all waves, one line per batch
    fprintf(stderr, "tm_phase_cycles prologue=%llu loop=%llu readback=%llu sort=%llu ms_match=%.4f\n",
            b->walk.h_stats[ST_PHASE + 0], b->walk.h_stats[ST_PHASE + 1], b->walk.h_stats[ST_PHASE + 2], b->walk.h_stats[ST_PHASE + 3],
            ms_match);
#endif
}

int tm_engine::wait(tm_batch* b, bool drained, uint32_t* relaunched) {
    if (!b->launched) return TM_EINVAL;
    const hipStream_t S = st(b);
    if (!b->csr) {   // an async launch stopped after the walk: redo it the CSR way
        int rc = launch(b, true);
        if (rc) return rc;
        drained = false;
    }
    for (int attempt = 0;; ++attempt) {
        if (!drained || attempt) {
            if (b->end_recorded) HIP_OK(hipEventSynchronize(b->walk.ev_end.e));
            else HIP_OK(hipStreamSynchronize(S));
        }
        if (attempt && relaunched) ++*relaunched;
        if (b->dedup_dev) {   // the walk's rows: the distinct publishes counted by the dedup pass
            b->n = b->walk.h_ctrl[CTRL_NROWS];
            b->scan_args.n = b->n;
        }
        if (b->check_tokens && b->n && b->tok.h_bad.p[1]) {
            snprintf(last_error(), 512, "token batch failed the device check (word offsets or flags)");
            return TM_EINVAL;
        }
        const uint32_t* h_dbg = b->rep->tab.h_dbg.p;
        if (checked && h_dbg[0]) {
            snprintf(last_error(), 512, "bounds check %u failed: index %u bound %u (count %u, extra %u)",
                     h_dbg[0], h_dbg[1], h_dbg[2], h_dbg[3], h_dbg[4]);
            return TM_EIO;
        }
        uint32_t err;
        uint64_t need, staged;
        int rc = check_ctrl(b->walk.h_ctrl, b->walk.h_stats, &err, &need, &staged);
        if (rc) return rc;
        if (!err) break;
        if (attempt >= 6) {
            snprintf(last_error(), 512, "capacity misses did not settle after %d relaunches (err %#x, %llu staged)",
                     attempt, err, (unsigned long long)staged);
            return TM_EOVERFLOW;
        }
        if ((rc = grow_for(b, err, need, staged))) return rc;
        if ((rc = launch(b))) return rc;
    }
    fill_stats(b);
    b->done = true;
    if (b->dedup_dev) b->dtab_dirty = false;   // (its expansion cleared the claimed slots)
    // (dense_enq, not eager_dense: the pipelined caller clears eager_dense
    // right after launch, while the tail it asked for is already queued)
    b->dense = b->dense_enq && !b->oneshot && b->total <= b->dense_cap;
    if (b->dense) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, b->dcsr.evc0.e, b->dcsr.evc1.e);
        b->st.ms_csr = ms;
    }
    return TM_OK;
}

int tm_engine::result(tm_batch* b, tm_result* out) {
    if (!b->done) return TM_EINVAL;
    int rc;
    if ((rc = ensure_dense(b))) return rc;
    const hipStream_t S = st(b);
    // the match count is known since wait(): both copies go out behind one sync
    const uint64_t total = b->total;
    if (total > b->dcsr.d_ids.cap) {
        snprintf(last_error(), 512, "inconsistent CSR: kernel count %llu, capacity %zu",
                 (unsigned long long)total, b->dcsr.d_ids.cap);
        return TM_EIO;
    }
    if ((rc = b->dcsr.h_rowoff.reserve((size_t)b->n + 1))) return rc;
    if ((rc = b->dcsr.h_ids.reserve(std::max<uint64_t>(total, 1)))) return rc;
    HIP_OK(hipMemcpyAsync(b->dcsr.h_rowoff.p, b->dcsr.d_rowoff.p, ((size_t)b->n + 1) * 4, hipMemcpyDeviceToHost, S));
    if (total) HIP_OK(hipMemcpyAsync(b->dcsr.h_ids.p, b->dcsr.d_ids.p, total * 4, hipMemcpyDeviceToHost, S));
    HIP_OK(hipStreamSynchronize(S));
    if (b->dcsr.h_rowoff.p[b->n] != total) {
        snprintf(last_error(), 512, "inconsistent CSR: row offsets end at %u, kernel count %llu",
                 b->dcsr.h_rowoff.p[b->n], (unsigned long long)total);
        return TM_EIO;
    }
    out->n_topics = b->n;
    out->n_matches = total;
    out->row_offsets = b->dcsr.h_rowoff.p;
    out->filter_ids = b->dcsr.h_ids.p;
    return TM_OK;
}

// tm_result with the ids packed to 3 bytes on the device (while the trie's
// node ids fit 24 bits), copied into the batch's own pinned buffer: a quarter
// less D2H and nothing to unpack on the host (tm_filters_copy_packed reads them)
int tm_engine::result_packed(tm_batch* b, tm_result_packed* out) {
    if (nd.size() > (1u << 24)) {   // 4-byte ids: the plain result
        tm_result r{};
        int rc = result(b, &r);
        if (rc) return rc;
        out->n_topics = r.n_topics;
        out->id_bytes = 4;
        out->n_matches = r.n_matches;
        out->row_offsets = r.row_offsets;
        out->ids = reinterpret_cast<const uint8_t*>(r.filter_ids);
        return TM_OK;
    }
    if (!b->done) return TM_EINVAL;
    int rc;
    if ((rc = ensure_dense(b))) return rc;
    const hipStream_t S = st(b);
    const uint64_t total = b->total;
    if (total > b->dcsr.d_ids.cap) {
        snprintf(last_error(), 512, "inconsistent CSR: kernel count %llu, capacity %zu",
                 (unsigned long long)total, b->dcsr.d_ids.cap);
        return TM_EIO;
    }
    if ((rc = b->dcsr.h_rowoff.reserve((size_t)b->n + 1))) return rc;
    if ((rc = b->dcsr.h_ids8.reserve((size_t)total * 3 + 16))) return rc;
    HIP_OK(hipMemcpyAsync(b->dcsr.h_rowoff.p, b->dcsr.d_rowoff.p, ((size_t)b->n + 1) * 4, hipMemcpyDeviceToHost, S));
    if (total) {
        if ((rc = b->dcsr.d_pack.reserve(total * 3 + 16))) return rc;
        HIP_OK(launch_pack_ids(b->dcsr.d_ids.p, total, b->dcsr.d_pack.p, S));
        HIP_OK(hipMemcpyAsync(b->dcsr.h_ids8.p, b->dcsr.d_pack.p, total * 3, hipMemcpyDeviceToHost, S));
    }
    HIP_OK(hipStreamSynchronize(S));
    if (b->dcsr.h_rowoff.p[b->n] != total) {
        snprintf(last_error(), 512, "inconsistent CSR: row offsets end at %u, kernel count %llu",
                 b->dcsr.h_rowoff.p[b->n], (unsigned long long)total);
        return TM_EIO;
    }
    out->n_topics = b->n;
    out->id_bytes = 3;
    out->n_matches = total;
    out->row_offsets = b->dcsr.h_rowoff.p;
    out->ids = b->dcsr.h_ids8.p;
    return TM_OK;
}

int tm_engine::sample(tm_batch* b, const uint32_t* rows, uint32_t k, tm_result* out) {
    if (!b->done || !b->csr) return TM_EINVAL;
    for (uint32_t i = 0; i < k; ++i)
        if (rows[i] >= b->n) return TM_EINVAL;
    const hipStream_t S = st(b);
    b->h_smp_off.assign((size_t)k + 1, 0);
    b->h_smp_ids.clear();
    if (k) {
        int rc;
        // [rows u32 k | cnt u32 k | pad | src u64 k | off u64 k + 1], batch-owned
        const size_t o_src = (((size_t)k * 8) + 15) & ~(size_t)15, o_off = o_src + (size_t)k * 8;
        if ((rc = b->smp.d_smp_meta.reserve(o_off + ((size_t)k + 1) * 8))) return rc;
        uint8_t* m = b->smp.d_smp_meta.p;
        uint32_t* d_rows = reinterpret_cast<uint32_t*>(m);
        uint32_t* d_cnt = d_rows + k;
        unsigned long long* d_src = reinterpret_cast<unsigned long long*>(m + o_src);
        uint64_t* d_off = reinterpret_cast<uint64_t*>(m + o_off);
        std::vector<uint32_t> cnt(k);
        HIP_OK(hipMemcpyAsync(d_rows, rows, (size_t)k * 4, hipMemcpyHostToDevice, S));
        HIP_OK(launch_sample_meta(b->walk.d_count, b->walk.d_src, d_rows, k, d_cnt, d_src, S));
        HIP_OK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)k * 4, hipMemcpyDeviceToHost, S));
        HIP_OK(hipStreamSynchronize(S));
        std::vector<uint64_t> off((size_t)k + 1, 0);
        for (uint32_t i = 0; i < k; ++i) off[i + 1] = off[i] + cnt[i];
        if (off[k] > MAX_RESULT) return TM_EOVERFLOW;   // u32 CSR offsets
        for (uint32_t i = 0; i <= k; ++i) b->h_smp_off[i] = (uint32_t)off[i];
        b->h_smp_ids.resize(off[k]);
        if (off[k]) {
            if ((rc = b->smp.d_smp_ids.reserve(off[k]))) return rc;
            HIP_OK(hipMemcpyAsync(d_off, off.data(), off.size() * 8, hipMemcpyHostToDevice, S));
            HIP_OK(launch_sample_ids(b->walk.d_sfids.p, d_cnt, d_src, d_off, k, b->smp.d_smp_ids.p, S));
            HIP_OK(hipMemcpyAsync(b->h_smp_ids.data(), b->smp.d_smp_ids.p, off[k] * 4, hipMemcpyDeviceToHost, S));
            HIP_OK(hipStreamSynchronize(S));
        }
    }
    if (b->h_smp_ids.empty()) b->h_smp_ids.push_back(0);   // (a valid pointer for an empty result)
    out->n_topics = k;
    out->n_matches = b->h_smp_off[k];
    out->row_offsets = b->h_smp_off.data();
    out->filter_ids = b->h_smp_ids.data();
    return TM_OK;
}
