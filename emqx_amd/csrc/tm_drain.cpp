// tm_drain.cpp -- the session drain (tm_sessions_drain): emqx_session:dequeue/1
// with message expiry over the queued messages of a batch of sessions.  The
// host checks the call, leaves the empty sessions out (a session the kernels
// see owns at least one message), sends the arrays up, and puts the
// per-session results back at the caller's session indices.
#include "tm_engine_impl.hpp"

static_assert(DRAIN_NDISP == TM_DRAIN_COUNT && DRAIN_BATCH_N == TM_DRAIN_BATCH_N && DRAIN_EXPIRY == TM_QMSG_EXPIRY &&
                  PRIO_CLASSES == TM_PRIO_MAX_CLASSES && TM_QMSG_CLASS_SHIFT == 4,
              "the kernels' constants are the header's");
static_assert(sizeof(tm_drain_session) == sizeof(uint2) && sizeof(tm_drain_record) == sizeof(uint4),
              "the kernels read and write the public structs as vectors");

namespace {

// every TM_EINVAL of the call; *ncls = the highest class of the messages + 1
int drain_check(const tm_drain_in* in, const tm_drain_out* out, uint32_t* ncls) {
    if (!in) return einval("tm_sessions_drain: in is NULL");
    if (!out) return einval("tm_sessions_drain: out is NULL");
    if (in->pad0) return einval("tm_sessions_drain: pad0 = %u", in->pad0);
    const uint32_t n = in->n_sessions;
    *ncls = 1;
    if (!n) return TM_OK;
    if (!in->sessions) return einval("tm_sessions_drain: sessions is NULL");
    if (!in->q_off) return einval("tm_sessions_drain: q_off is NULL");
    if (!out->records) return einval("tm_sessions_drain: records is NULL");
    if (!out->popped) return einval("tm_sessions_drain: popped is NULL");
    for (uint32_t r = 0; r < n; ++r) {
        const uint32_t p = in->sessions[r].next_pkt_id;
        if (p < 1 || p > 65535) return einval("tm_sessions_drain: session %u: next_pkt_id %u outside 1..65535", r, p);
        if (in->q_off[r + 1] < in->q_off[r])
            return einval("tm_sessions_drain: session %u: offsets not monotone (%llu after %llu)", r,
                          (unsigned long long)in->q_off[r + 1], (unsigned long long)in->q_off[r]);
    }
    if (in->q_off[0]) return einval("tm_sessions_drain: q_off[0] = %llu, not 0", (unsigned long long)in->q_off[0]);
    const uint64_t Q = in->q_off[n];
    if (Q >= (1ull << 32)) return einval("tm_sessions_drain: %llu messages, not below 2^32", (unsigned long long)Q);
    if (!Q) return TM_OK;
    if (!in->qmsg) return einval("tm_sessions_drain: qmsg is NULL");
    if (!out->disp) return einval("tm_sessions_drain: disp is NULL");
    if (!out->packet_ids) return einval("tm_sessions_drain: packet_ids is NULL");
    if (!out->order) return einval("tm_sessions_drain: order is NULL");
    // one pass that the compiler vectorises; the offender is looked for only when there is one
    uint32_t any = 0, q3 = 0, top = 0;
    for (uint64_t m = 0; m < Q; ++m) {
        const uint32_t b = in->qmsg[m];
        any |= b;
        q3 |= (b & (b >> 1)) & 1u;
        top = std::max(top, b & 0x70u);
    }
    const bool arrays = in->created_ms && in->expiry_s;
    if ((any & DRAIN_RESERVED) || q3 || ((any & TM_QMSG_EXPIRY) && !arrays))
        for (uint64_t m = 0; m < Q; ++m) {
            const uint32_t b = in->qmsg[m];
            if ((b & 3u) == 3u) return einval("tm_sessions_drain: message %llu: QoS 3", (unsigned long long)m);
            if (b & DRAIN_RESERVED)
                return einval("tm_sessions_drain: message %llu: reserved bits set (qmsg = 0x%02x)", (unsigned long long)m, b);
            if ((b & TM_QMSG_EXPIRY) && !arrays)
                return einval("tm_sessions_drain: message %llu has TM_QMSG_EXPIRY but %s is NULL", (unsigned long long)m,
                              in->created_ms ? "expiry_s" : "created_ms");
        }
    *ncls = (top >> TM_QMSG_CLASS_SHIFT) + 1;
    return TM_OK;
}

int drain_run(tm_engine* e, Replica& R, const tm_drain_in* in, tm_drain_out* out, uint32_t ncls) {
    Replica::Drain& D = R.drain;
    const hipStream_t s = R.stream;
    const uint32_t n = in->n_sessions;
    const uint64_t Q = in->q_off[n];
    // a session without messages: dequeue/1's first clause (src/emqx_session.erl:390-391)
    for (uint32_t r = 0; r < n; ++r) out->records[r] = tm_drain_record{in->sessions[r].next_pkt_id, 0u, 0u, 0u};
    memset(out->popped, 0, (size_t)n * TM_PRIO_MAX_CLASSES * sizeof(uint32_t));
    if (!Q) return TM_OK;
    int rc;
    // the sessions that own a message, in order: their first message and state
    if ((rc = D.off.h.reserve((size_t)n + 1))) return rc;
    if ((rc = D.sess.h.reserve(n))) return rc;
    std::vector<uint32_t> ne;   // their indices in the call; empty when no session was left out
    uint32_t Rn = 0;
    for (uint32_t r = 0; r < n; ++r)
        if (in->q_off[r + 1] > in->q_off[r]) {
            D.off.h.p[Rn] = (uint32_t)in->q_off[r];
            D.sess.h.p[Rn] = make_uint2(in->sessions[r].next_pkt_id, in->sessions[r].inflight_free);
            ++Rn;
        }
    D.off.h.p[Rn] = (uint32_t)Q;
    if (Rn != n) {
        ne.reserve(Rn);
        for (uint32_t r = 0; r < n; ++r)
            if (in->q_off[r + 1] > in->q_off[r]) ne.push_back(r);
    }
    const bool exp_in = in->created_ms && in->expiry_s;
    const uint32_t ntiles = (uint32_t)((Q + INBOX_TILE - 1) / INBOX_TILE), nwaves = ntiles * 4;
    const size_t nsb = (nwaves + PRIO_SCAN_TILE - 1) / PRIO_SCAN_TILE;
    const size_t nheads = 2 * (size_t)((Q + 63) / 64) + 2;
    if ((rc = D.off.d.reserve((size_t)Rn + 1))) return rc;
    if ((rc = D.sess.d.reserve(Rn))) return rc;
    if ((rc = D.d_qmsg.reserve(Q))) return rc;
    if ((rc = D.d_kind.reserve(Q))) return rc;
    if (exp_in && (rc = D.d_created.reserve(Q))) return rc;
    if (exp_in && (rc = D.d_expiry.reserve(Q))) return rc;
    if (out->expiry_out && (rc = D.d_expout.reserve(Q))) return rc;
    if ((rc = D.d_disp.reserve(Q))) return rc;
    if ((rc = D.d_pid.reserve(Q))) return rc;
    if ((rc = D.d_order.reserve(Q))) return rc;
    if ((rc = D.d_heads.reserve(nheads))) return rc;
    if ((rc = D.d_chbase.reserve((size_t)Rn * DRAIN_COLS))) return rc;
    if ((rc = D.d_cw.reserve(((size_t)nwaves + 1) * DRAIN_COLS))) return rc;
    if ((rc = D.d_cbs.reserve((nsb + 1) * DRAIN_COLS))) return rc;
    if ((rc = D.d_ctot.reserve(DRAIN_COLS))) return rc;
    if ((rc = D.d_wdisp.reserve((size_t)nwaves * DRAIN_NDISP))) return rc;
    if ((rc = D.d_plan.reserve((size_t)Rn * PRIO_CLASSES))) return rc;
    if ((rc = D.popped.reserve((size_t)Rn * PRIO_CLASSES))) return rc;
    if ((rc = D.rec.reserve(Rn))) return rc;
    if ((rc = D.tot.reserve(DRAIN_NDISP + 1))) return rc;
    if ((rc = D.ev0.create())) return rc;
    if ((rc = D.ev1.create())) return rc;
    HIP_OK(hipMemcpyAsync(D.off.d.p, D.off.h.p, ((size_t)Rn + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(D.sess.d.p, D.sess.h.p, (size_t)Rn * sizeof(uint2), hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(D.d_qmsg.p, in->qmsg, Q, hipMemcpyHostToDevice, s));
    if (exp_in) {
        HIP_OK(hipMemcpyAsync(D.d_created.p, in->created_ms, Q * sizeof(int64_t), hipMemcpyHostToDevice, s));
        HIP_OK(hipMemcpyAsync(D.d_expiry.p, in->expiry_s, Q * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    HIP_OK(hipMemsetAsync(D.d_heads.p, 0, nheads * sizeof(uint32_t), s));
    HIP_OK(hipMemsetAsync(D.tot.d.p, 0, (DRAIN_NDISP + 1) * sizeof(unsigned long long), s));
    DrainArgs a{};
    a.off = D.off.d.p; a.sess = D.sess.d.p; a.qmsg = D.d_qmsg.p;
    a.created = exp_in ? D.d_created.p : nullptr; a.expiry = exp_in ? D.d_expiry.p : nullptr;
    a.now_ms = in->now_ms;
    a.Q = (uint32_t)Q; a.R = Rn; a.nwaves = nwaves; a.ncls = ncls;
    a.heads = D.d_heads.p; a.kind = D.d_kind.p; a.chbase = D.d_chbase.p; a.cw = D.d_cw.p; a.cbs = D.d_cbs.p;
    a.ctot = D.d_ctot.p; a.plan = D.d_plan.p;
    a.disp = D.d_disp.p; a.pid = D.d_pid.p; a.order = D.d_order.p;
    a.expiry_out = out->expiry_out ? D.d_expout.p : nullptr;
    a.rec = D.rec.d.p; a.popped = D.popped.d.p; a.wdisp = D.d_wdisp.p;
    a.totals = D.tot.d.p; a.bad = reinterpret_cast<uint32_t*>(D.tot.d.p + DRAIN_NDISP);
    HIP_OK(hipEventRecord(D.ev0.e, s));
    HIP_OK(launch_drain(a, s));
    HIP_OK(hipEventRecord(D.ev1.e, s));
    HIP_OK(hipMemcpyAsync(out->disp, D.d_disp.p, Q, hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out->packet_ids, D.d_pid.p, Q * sizeof(uint16_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(out->order, D.d_order.p, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (out->expiry_out)
        HIP_OK(hipMemcpyAsync(out->expiry_out, D.d_expout.p, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if ((rc = D.rec.fetch(Rn, s))) return rc;
    if ((rc = D.popped.fetch((size_t)Rn * PRIO_CLASSES, s))) return rc;
    if ((rc = D.tot.fetch(DRAIN_NDISP + 1, s))) return rc;
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipEventElapsedTime(&out->kernel_ms, D.ev0.e, D.ev1.e));
    const uint32_t bad = (uint32_t)D.tot.h.p[DRAIN_NDISP];
    if (bad) {
        snprintf(last_error(), 512, "tm_sessions_drain: %u indices past the messages or the sessions", bad);
        return TM_EIO;
    }
    for (uint32_t k = 0; k < TM_DRAIN_COUNT; ++k) out->totals[k] = D.tot.h.p[k];
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "totals are copied as they are");
    if (ne.empty()) {
        memcpy(out->records, D.rec.h.p, (size_t)Rn * sizeof(tm_drain_record));
        memcpy(out->popped, D.popped.h.p, (size_t)Rn * PRIO_CLASSES * sizeof(uint32_t));
    } else {
        for (uint32_t k = 0; k < Rn; ++k) {
            memcpy(&out->records[ne[k]], &D.rec.h.p[k], sizeof(tm_drain_record));
            memcpy(out->popped + (size_t)ne[k] * PRIO_CLASSES, D.popped.h.p + (size_t)k * PRIO_CLASSES,
                   PRIO_CLASSES * sizeof(uint32_t));
        }
    }
    (void)e;
    return TM_OK;
}

}  // namespace

int tm_sessions_drain(tm_engine* e, const tm_drain_in* in, tm_drain_out* out) {
    if (!e) return TM_EINVAL;
    uint32_t ncls = 1;
    if (int rc = drain_check(in, out, &ncls)) return rc;
    if (e->reps.empty()) return TM_ENODEV;   // host-only engine: no CPU fallback
    for (uint64_t& t : out->totals) t = 0;
    out->kernel_ms = 0.f;
    out->pad0 = 0;
    if (!in->n_sessions) return TM_OK;
    std::lock_guard<std::recursive_mutex> g(e->mu);
    if (int rc = e->set_device()) return rc;   // the first replica
    try {
        return drain_run(e, *e->reps[0], in, out, ncls);
    } catch (...) {
        return TM_ENOMEM;
    }
}
