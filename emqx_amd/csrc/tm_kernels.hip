// tm_kernels.hip -- gfx950 (CDNA4) kernels of the topic-matching engine.
//
// The reference walk is emqx_trie:match/1 -> match_node/3 (src/emqx_trie.erl:
// 96-99, 162-186): per visited node, emit its '#' child's topic, then follow the
// literal word and the '+' edge; at the end of the words emit the node's own
// topic and its '#' child's.  Here that recursion becomes a frontier expansion:
//
//   tm_match_tiles  one 64-lane wavefront owns a TILE of 64 topics.  Pending
//                   edge probes of all 64 topics live in an LDS stack; every
//                   iteration pops up to 64 of them (one per lane), each lane
//                   reads ONE 64-B hash bucket whose matching 16-B slot holds the
//                   child's whole summary, and the lanes push their children
//                   through ballot + mbcnt prefix sums.  Each match is one u64
//                   (3-bit-per-level path code | filter id) stored into the
//                   topic's row of the wave's private emission buffer; path-code
//                   order == Erlang binary order of the filters (DESIGN.md "Sort
//                   order").  When the tile's frontier is empty the wave sorts
//                   its 64 rows in registers (bitonic over __shfl_xor) and
//                   stages the filter ids as ONE contiguous run per tile.
//   tm_match_slow   one wavefront per topic, frontier in global scratch: deep
//                   (> 10 levels) or irregular topics (sorted by filter bytes),
//                   rows longer than K and tiles whose LDS stack overflowed.
//   scan            exclusive scan of the per-topic counts -> CSR offsets.
//   tm_finalize     one wave per tile: a tile's staged run is copied into the
//                   CSR with coalesced loads/stores (per-topic copy for tiles
//                   holding slow-path topics).
//
// No MFMA: this is a dependent irregular gather, bound by the memory system.
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include "tm_internal.hpp"

namespace etm {

constexpr int TILE = 64;
constexpr int WCAP = 512;   // LDS word cache per tile
#ifndef TM_WPE384
#define TM_WPE384 4         // waves/SIMD the 384-entry-stack kernel is register-allocated for
#endif

// queue/meta encoding (fast path): tl (6 bits) | lc << 6 (4 bits, lc <= FAST_MAX_DEPTH) | flags.
// It rides in the low 31 bits of the probe's path-code key, which are zero
// until a filter id is put there at emission.
constexpr uint32_t M_LVL_SHIFT = 6;
constexpr uint32_t M_LVL_MASK = 0xF;
constexpr uint32_t M_PLUS = 1u << 10;    // probe the '+' edge (else the literal word w[lc-1])
constexpr uint32_t M_SKIPE = 1u << 11;   // don't emit the child's own topic (literal '#' dup)
constexpr uint32_t M_DSTART = 1u << 12;  // $-rooted start probe: the node was already counted
static_assert(FAST_MAX_DEPTH <= (int)M_LVL_MASK, "level field too narrow");
constexpr uint32_t M_DISP_SHIFT = 13;    // bucket displacement of a continued probe (<= max_probe <= MAX_PROBE_DISP)
constexpr uint32_t M_DISP_MASK = 0x3F;
static_assert(MAX_PROBE_DISP <= M_DISP_MASK, "the displacement field holds every bounded probe run");
// How a quad of lanes serves a probe's owner lane in the frontier loop (A/B
// builds: python -m emqx_amd.build --variant NAME -DTM_QUAD_OWN=n):
//   1  the owner sits in the quad that reads its bucket: the request reaches
//      the quad by DPP, the found slot goes back whole (one ds_write_b128)
//   2  the DPP requests of 1 with the report of 0 (measurement only)
//   0  the protocol of rounds 1-10: probe 16r + q, request and report through
//      the owner's LDS entry, field by field
#ifndef TM_QUAD_OWN
#define TM_QUAD_OWN 1
#endif
#if TM_QUAD_OWN != 1
// probe-entry marks written by the quad: FOUND | the child's literal signature
// into the parent field, TAIL into the word field (never a parent / word id)
constexpr uint32_t Q_FOUND = ~((1u << LSIG_BITS) - 1u);
constexpr uint32_t Q_TAIL = 0xFFFFFFFFu;
#endif
// A lane without a probe offers its quad this byte offset into the slot table:
// with the three slots after it, it lies past every table that is read with
// buffer loads (launch_match), so the loads return 0 without a memory access.
constexpr uint32_t OFF_NONE = 0xFFFFFFC0u;

// digit tables indexed by class (C_BELOW, C_BETWEEN, C_ABOVE, C_EMPTY):
//   L = literal branch, H = '#' terminal, P = '+' branch; E = 0, L_lo = 1.
__device__ __forceinline__ uint32_t dig_L(uint32_t c) { return (0x4432u >> (4 * c)) & 0xF; }
__device__ __forceinline__ uint32_t dig_H(uint32_t c) { return (0x2223u >> (4 * c)) & 0xF; }
__device__ __forceinline__ uint32_t dig_P(uint32_t c) { return (0x3344u >> (4 * c)) & 0xF; }

__device__ __forceinline__ int key_shift(uint32_t level) { return 61 - 3 * (int)level; }

__device__ __forceinline__ uint64_t put_digit(uint64_t key, uint32_t level, uint32_t d) {
    return level <= FAST_MAX_DEPTH ? (key | ((uint64_t)d << key_shift(level))) : key;
}

__device__ __forceinline__ uint32_t prefix_count(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Bounds-checked debug variant: an out-of-range index is recorded (first
// failing check id, index, bound) and clamped to 0 instead of faulting.
template <bool CK>
__device__ __forceinline__ uint64_t ck(uint64_t i, uint64_t bound, uint32_t* dbg, uint32_t id) {
    if (CK && i >= bound) {
        if (dbg) {
            if (atomicCAS(&dbg[0], 0u, id) == 0u) { dbg[1] = (uint32_t)i; dbg[2] = (uint32_t)bound; }
            atomicAdd(&dbg[3], 1u);
        }
        return 0;
    }
    return i;
}
#define CK_(i, bound, id) ck<CK>((i), (bound), a.dbg, (id))

// Child summary decoded from one slot.
struct Node {
    uint32_t child;   // node id
    uint32_t term;    // own filter id or NONE
    uint32_t hterm;   // filter id of child/'#' or NONE
    uint32_t flags;   // NF_*
};

// One 64-B bucket read (four 16-B slots, key compare).  max_probe bounds the scan.
// Tables under 4 GiB are read with raw buffer loads (a wave-uniform descriptor
// built from kernel arguments): four dwordx4 that the compiler cannot narrow,
// issued back to back.  Larger tables use plain global loads.
#ifndef TM_PROBE_CPOL
#define TM_PROBE_CPOL 0     // cache-policy bits of the bucket loads (gfx950: 1 = sc0, 2 = nt, 16 = sc1)
#endif
__device__ __forceinline__ uint4 ld_b128(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, TM_PROBE_CPOL);
    return uint4{v[0], v[1], v[2], v[3]};
}

template <bool CK, bool BIG>
__device__ __forceinline__ bool probe(const MatchArgs& a, uint32_t parent, uint32_t word, Node& n) {
    uint32_t b = home_bucket(parent, word, a.nbuckets);
    const bool small = !BIG;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<Slot*>(a.slots), 0, BIG ? 0u : a.nslots * 16u, 0x00020000);
    for (uint32_t p = 0; p <= a.max_probe; ++p) {
        uint4 s0, s1, s2, s3;
        const uint64_t si = CK_((uint64_t)b * BUCKET, a.nslots, 1);
        if (small) {
            const uint32_t off = (uint32_t)si * 16u;
            s0 = ld_b128(rs, off); s1 = ld_b128(rs, off + 16); s2 = ld_b128(rs, off + 32); s3 = ld_b128(rs, off + 48);
        } else {
            const uint4* q = reinterpret_cast<const uint4*>(a.slots) + si;
            s0 = q[0]; s1 = q[1]; s2 = q[2]; s3 = q[3];
        }
        // (the key's top bits are the child's literal signature)
        const bool m0 = (s0.x & ID_MASK) == parent && (s0.y & WID_MASK) == word;
        const bool m1 = (s1.x & ID_MASK) == parent && (s1.y & WID_MASK) == word;
        const bool m2 = (s2.x & ID_MASK) == parent && (s2.y & WID_MASK) == word;
        const bool m3 = (s3.x & ID_MASK) == parent && (s3.y & WID_MASK) == word;
        const uint32_t hz = m0 ? s0.z : m1 ? s1.z : m2 ? s2.z : s3.z;
        const uint32_t hw = m0 ? s0.w : m1 ? s1.w : m2 ? s2.w : s3.w;
        if (m0 | m1 | m2 | m3) {
            n.child = hz & ID_MASK;
            n.term = (hz & B_TOPIC) ? n.child : NONE;
            n.hterm = (hw & B_HTERM) ? (hw & ID_MASK) : NONE;
            n.flags = ((hz & B_PLUS) ? NF_PLUS : 0u) | ((hw & B_HASH) ? NF_HASH : 0u);
            return true;
        }
        if (s3.x == SLOT_EMPTY) return false;   // slots fill in order: a free tail ends the run
        b = (b + 1 == a.nbuckets) ? 0 : b + 1;
    }
    return false;
}

// Expansion of one found child at level lc (= words consumed), mirroring
// match_node/3: at the end of the words the node's own topic and its '#'
// child's (src/emqx_trie.erl:168-169); otherwise the '#' child's topic, then the
// literal and '+' probes (:171-177).
struct Expand {
    uint32_t ne, np;
    uint32_t ef0, ef1;
    uint64_t ek0, ek1;
    uint32_t pf0, pf1;     // M_PLUS / M_SKIPE / M_DSTART
    uint64_t pk0, pk1;
};

__device__ __forceinline__ void add_e(Expand& x, uint32_t fid, uint64_t key) {
    if (x.ne == 0) { x.ef0 = fid; x.ek0 = key; } else { x.ef1 = fid; x.ek1 = key; }
    x.ne++;
}
__device__ __forceinline__ void add_p(Expand& x, uint64_t key, uint32_t fl) {
    if (x.np == 0) { x.pk0 = key; x.pf0 = fl; } else { x.pk1 = key; x.pf1 = fl; }
    x.np++;
}

__device__ __forceinline__ void expand(const Node& s, uint32_t lc, uint32_t d, uint32_t flags,
                                       uint64_t key, uint32_t w_here, uint32_t w_prev, Expand& x) {
    x.ne = 0; x.np = 0;
    if (lc == d) {
        if (!(flags & M_SKIPE) && s.term != NONE) {
            uint64_t k = key;
            // '' word at level lc-1 followed by the end: "P/" sorts before "P/#".
            if ((w_prev >> WID_BITS) == C_EMPTY && lc - 1 <= FAST_MAX_DEPTH) {
                const int sp = key_shift(lc - 1);
                if (((k >> sp) & 7) == 4) k = (k & ~(7ull << sp)) | (1ull << sp);
            }
            add_e(x, s.term, k);
        }
        if (s.hterm != NONE) add_e(x, s.hterm, put_digit(key, lc, 2));
        return;
    }
    const uint32_t cls = w_here >> WID_BITS, id = w_here & WID_MASK;
    if (s.hterm != NONE) add_e(x, s.hterm, put_digit(key, lc, dig_H(cls)));
    if (id == W_HASH) {
        if (s.flags & NF_HASH) add_p(x, put_digit(key, lc, dig_L(cls)), (lc + 1 == d) ? M_SKIPE : 0u);
    } else if (id != W_UNKNOWN && id != W_PLUS) {
        add_p(x, put_digit(key, lc, dig_L(cls)), 0u);
    }
    if (s.flags & NF_PLUS) add_p(x, put_digit(key, lc, dig_P(cls)), M_PLUS);
}

// Root expansion for a topic (match_node(root, Words), or the $ rule that
// starts at node W and never tries root's '+'/'#', src/emqx_trie.erl:162-166).
__device__ __forceinline__ void expand_root(const RootRec& r, bool dollar, uint32_t d, uint32_t w0, Expand& x) {
    x.ne = 0; x.np = 0;
    const uint32_t cls = w0 >> WID_BITS, id = w0 & WID_MASK;
    if (!dollar && r.hterm != NONE) add_e(x, r.hterm, (uint64_t)dig_H(cls) << 61);
    if (id == W_HASH) {
        if (!dollar && (r.flags & NF_HASH)) add_p(x, (uint64_t)dig_L(cls) << 61, (d == 1) ? M_SKIPE : 0u);
    } else if (id != W_UNKNOWN && id != W_PLUS) {
        add_p(x, (uint64_t)dig_L(cls) << 61, dollar ? M_DSTART : 0u);
    }
    if (!dollar && (r.flags & NF_PLUS)) add_p(x, (uint64_t)dig_P(cls) << 61, M_PLUS);
}

// Per-wave LDS of the tile kernel.  The probe stack holds QC 16-B entries
// {key lo | meta, key hi, parent, word to probe (the literal w[lc-1] or
// W_PLUS / W_HASH)}: one ds_write_b128 per push, one ds_read_b128 per pop.
template <int QC>
struct alignas(16) TileLds {
    static constexpr int QCAP = QC;
    uint4 q[QC];
    uint32_t words[WCAP];
    uint32_t toff[TILE];
    uint32_t depth[TILE];
    uint32_t cnt[TILE];
    uint32_t list[TILE];
    // the stack and the word cache are free once a tile's frontier is empty: the
    // epilogue reuses them as a staging area of STAGE u64
    static constexpr uint32_t STAGE = (QC * 16 + WCAP * 4) / 8;
};

__device__ __forceinline__ uint4 q_pack(uint64_t key, uint32_t meta, uint32_t parent, uint32_t pw) {
    return uint4{(uint32_t)key | meta, (uint32_t)(key >> 32), parent, pw};
}

static_assert(offsetof(TileLds<512>, words) + sizeof(uint32_t) * WCAP == TileLds<512>::STAGE * 8,
              "staging area must be contiguous");
static_assert(offsetof(TileLds<384>, words) + sizeof(uint32_t) * WCAP == TileLds<384>::STAGE * 8,
              "staging area must be contiguous");

// Lane exchange with lane ^ j in VALU (no LDS crossbar): DPP quad_perm for 1
// and 2, row_half_mirror + quad reverse for 4, row_ror:8 for 8, and gfx950's
// v_permlane16/32_swap for 16 and 32.  j is a compile-time constant after the
// bitonic loops unroll, so the switch folds (tools/shx_check.hip checks all six).
__device__ __forceinline__ uint32_t xor_lane32(uint32_t v, uint32_t j) {
    const uint32_t lane = threadIdx.x & 63;
    switch (j) {
    case 1: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, false);
    case 2: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, false);
    case 4: return (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, false), 0x1B, 0xF,
                                                      0xF, false);
    case 8: return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, false);
    case 16: {
        const auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false);
        return (lane & 16) ? p[0] : p[1];
    }
    default: {
        const auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (lane & 32) ? p[0] : p[1];
    }
    }
}

__device__ __forceinline__ unsigned long long xor_lane64(unsigned long long v, uint32_t j) {
    return ((unsigned long long)xor_lane32((uint32_t)(v >> 32), j) << 32) | xor_lane32((uint32_t)v, j);
}

// Sum of a value over the wave's 64 lanes, wave-uniform (the per-lane values
// of one tile: far below 2^32 / 64 each).
__device__ __forceinline__ uint32_t tile_sum(uint32_t v) {
#pragma unroll
    for (uint32_t j = 1; j < 64; j <<= 1) v += xor_lane32(v, j);
    return __builtin_amdgcn_readfirstlane(v);
}

// Per-wave cycle sums of a tile's four phases (-DTM_PHASE_CYCLES=1, dev builds
// only: python -m emqx_amd.build --variant phase -DTM_PHASE_CYCLES=1).  The
// sums leave with the wave's wstats partials and fill_stats prints them.  In
// the default build the struct is empty and its calls compile to nothing.
enum : int { PH_PROLOGUE = 0, PH_LOOP = 1, PH_READBACK = 2, PH_SORT = 3 };
struct PhaseClk {
#if TM_PHASE_CYCLES
    unsigned long long sum[PHASE_N] = {0, 0, 0, 0}, t0 = 0;
    __device__ __forceinline__ void start() { t0 = __builtin_readcyclecounter(); }
    __device__ __forceinline__ void lap(int p) {
        const unsigned long long now = __builtin_readcyclecounter();
        sum[p] += now - t0;
        t0 = now;
    }
#else
    __device__ __forceinline__ void start() {}
    __device__ __forceinline__ void lap(int) {}
#endif
};

// xor_lane32 for j <= 8 with bound_ctrl set (every lane has a source, so the
// value is the same): the form the compiler folds into the v_min / v_max that
// use it as their DPP operand
__device__ __forceinline__ uint32_t xor_lane32_bc(uint32_t v, uint32_t j) {
    const int x = (int)v;
    switch (j) {
    case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);
    case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true);
    case 4: return (uint32_t)__builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true),
                                                         0x1B, 0xF, 0xF, true);
    default: return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, true);
    }
}

// The value of lane r of each quad in all four of its lanes: DPP
// quad_perm:[r,r,r,r].  r is a compile-time constant once the rounds unroll.
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v, uint32_t r) {
    const int x = (int)v;
    switch (r) {
    case 0: return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x00, 0xF, 0xF, true);
    case 1: return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x55, 0xF, 0xF, true);
    case 2: return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0xAA, 0xF, 0xF, true);
    default: return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0xFF, 0xF, 0xF, true);
    }
}

#ifndef TM_TAGGED_SORT
#define TM_TAGGED_SORT 1   // 0: every size class sorts u64 (A/B builds)
#endif
// Tagged 32-bit row sort.  When every entry of a chunk has zero bits below
// `free` in the high word of its path code (and a zero bit 31), a row of size
// class W with log2(W) <= free sorts as ONE u32 per lane: the code's high word
// with the entry's index in the row in the free bits.  Path codes are distinct
// within a row -- a code spells the branch taken at every level (literal / '+' /
// '#' terminal / end have different digits in every word class, and the ''
// re-digit 4 -> 1 takes a value no other branch of the C_EMPTY class has), a
// literal '#' word's duplicate is never emitted (M_SKIPE) and a literal '+'
// word is never probed as a literal, so two entries of one topic with one code
// would be one filter emitted twice -- hence the tag never decides a compare
// and the order is the u64 sort's (code, then filter id; merge_runs_out relies
// on the same fact).  A stage is v_min_u32 / v_max_u32 on the exchanged value
// plus one select on a compile-time lane mask: lane e keeps the lower value
// iff ((e & j) == 0) == ((e & kk) == 0).
constexpr uint64_t keep_lo_mask(uint32_t W, uint32_t kk, uint32_t j) {
    uint64_t m = 0;
    for (uint32_t l = 0; l < 64; ++l) {
        const uint32_t e = l & (W - 1);
        if (((e & j) == 0) == ((e & kk) == 0)) m |= 1ull << l;
    }
    return m;
}

template <uint32_t W, uint32_t KK, uint32_t J>
__device__ __forceinline__ uint32_t tag_stage(uint32_t k) {
    constexpr uint64_t M = keep_lo_mask(W, KK, J);
    uint32_t lo, hi;
    if constexpr (J >= 16) {
        // after the swap both lanes of a pair hold {own, partner} in {p[0], p[1]}
        const auto p = J == 16 ? __builtin_amdgcn_permlane16_swap(k, k, false, false)
                               : __builtin_amdgcn_permlane32_swap(k, k, false, false);
        lo = min(p[0], p[1]);
        hi = max(p[0], p[1]);
    } else {
        const uint32_t other = xor_lane32_bc(k, J);
        lo = min(k, other);
        hi = max(k, other);
    }
    return __builtin_amdgcn_inverse_ballot_w64(M) ? lo : hi;
}
template <uint32_t W, uint32_t KK, uint32_t J>
__device__ __forceinline__ uint32_t tag_merge(uint32_t k) {
    k = tag_stage<W, KK, J>(k);
    if constexpr (J > 1) k = tag_merge<W, KK, J / 2>(k);
    return k;
}
template <uint32_t W, uint32_t KK = 2>
__device__ __forceinline__ uint32_t tag_sort(uint32_t k) {
    k = tag_merge<W, KK, KK / 2>(k);
    if constexpr (KK < W) k = tag_sort<W, KK * 2>(k);
    return k;
}

#ifndef TM_SORT_KPL
#define TM_SORT_KPL 4   // tagged keys per lane of a row sort; 1: one key per lane, the code of rounds 7-11 (A/B builds)
// (2 compiles -- 101 VGPRs -- and passes tests/test_gpu_sort_lanes.py; it was never measured: the fallback had 4 not fitted)
#endif
static_assert(TM_SORT_KPL == 1 || TM_SORT_KPL == 2 || TM_SORT_KPL == 4, "TM_SORT_KPL: 1, 2 or 4");
// K tagged keys per lane.  Element e of a row sits in lane e / K of the row's
// W / K lanes, register e % K, so a wave pass sorts 64 K / W rows and an
// exchange at element distance < K is a v_min_u32 / v_max_u32 pair between two
// of the lane's own registers.  The network is the all-ascending bitonic one:
// the first step of the merge of KK elements compares e with its mirror e ^
// (KK - 1), the others e with e ^ J (J = KK / 4 .. 1), and the lower element
// always keeps the lower value -- no step has a direction that depends on the
// lane, so the in-register steps carry no select (the standard form's merges
// of 2 K and up alternate by lane and would need one per register).  A mirror
// across lanes pairs register i with register K - 1 - i of lane l ^ (KK / K -
// 1): one DPP (quad_perm / row_half_mirror / row_mirror) up to 16 lanes.  In
// every lane step, lane l keeps the lower values iff its bit D (the distance,
// or the mirror's upper bit) is clear: a compile-time mask.
constexpr uint64_t lane_lo_mask(uint32_t d) {
    uint64_t m = 0;
    for (uint32_t l = 0; l < 64; ++l)
        if ((l & d) == 0) m |= 1ull << l;
    return m;
}

// the value of lane l ^ X, X = 2^n - 1
template <uint32_t X>
__device__ __forceinline__ uint32_t mirror_lane32_bc(uint32_t v) {
    const int x = (int)v;
    if constexpr (X == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true);
    else if constexpr (X == 3) return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x1B, 0xF, 0xF, true);
    else if constexpr (X == 7) return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true);
    else if constexpr (X == 15) return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true);
    else if constexpr (X == 31) return mirror_lane32_bc<15>(xor_lane32(v, 16));
    else return mirror_lane32_bc<15>(xor_lane32(xor_lane32(v, 32), 16));
}

// one step between lanes: distance D (MIRROR: partner l ^ (2 D - 1), registers reversed)
template <uint32_t K, uint32_t D, bool MIRROR>
__device__ __forceinline__ void kpl_lane_stage(uint32_t (&k)[K]) {
    const bool keep_lo = __builtin_amdgcn_inverse_ballot_w64(lane_lo_mask(D));
    uint32_t o[K];
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) {
        uint32_t lo, hi;
        if constexpr (!MIRROR && D >= 16) {
            // after the swap both lanes of a pair hold {own, partner} in {p[0], p[1]}
            const auto p = D == 16 ? __builtin_amdgcn_permlane16_swap(k[i], k[i], false, false)
                                   : __builtin_amdgcn_permlane32_swap(k[i], k[i], false, false);
            lo = min(p[0], p[1]);
            hi = max(p[0], p[1]);
        } else {
            uint32_t other;
            if constexpr (MIRROR) other = mirror_lane32_bc<2 * D - 1>(k[K - 1 - i]);
            else other = xor_lane32_bc(k[i], D);
            lo = min(k[i], other);
            hi = max(k[i], other);
        }
        o[i] = keep_lo ? lo : hi;
    }
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) k[i] = o[i];
}

// the steps at distance J, J / 2 .. 1 of a merge
template <uint32_t K, uint32_t J>
__device__ __forceinline__ void kpl_clean(uint32_t (&k)[K]) {
    if constexpr (J >= K) {
        kpl_lane_stage<K, J / K, false>(k);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < K; ++i) {
            if (i & J) continue;
            const uint32_t lo = min(k[i], k[i | J]), hi = max(k[i], k[i | J]);
            k[i] = lo;
            k[i | J] = hi;
        }
    }
    if constexpr (J > 1) kpl_clean<K, J / 2>(k);
}

template <uint32_t K, uint32_t W, uint32_t KK = 2>
__device__ __forceinline__ void kpl_sort(uint32_t (&k)[K]) {
    if constexpr (KK > K) {
        kpl_lane_stage<K, KK / (2 * K), true>(k);
    } else {
#pragma unroll
        for (uint32_t i = 0; i < K; ++i) {
            const uint32_t p = i ^ (KK - 1);
            if (i > p) continue;
            const uint32_t lo = min(k[i], k[p]), hi = max(k[i], k[p]);
            k[i] = lo;
            k[p] = hi;
        }
    }
    if constexpr (KK >= 4) kpl_clean<K, KK / 4>(k);
    if constexpr (KK < W) kpl_sort<K, W, KK * 2>(k);
}

// One wave pass of the K-keys-per-lane sort: this lane holds elements K l ..
// K l + K - 1 of the row {cr, pr, dr} (rv: it has one).  Keys are the staged
// codes' high words with the element's index in the free bits, the padding
// 0xFFFFFFFF; sorted place e then holds the entry that arrived as number
// tag.
template <bool CK, uint32_t K, uint32_t W, uint32_t STAGE>
__device__ __forceinline__ void kpl_pass(const MatchArgs& a, const uint32_t* stg32, bool rv, uint32_t l, uint32_t cr,
                                         uint32_t pr, uint32_t dr) {
    uint32_t k[K];
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) {
        const uint32_t e = K * l + i;
        k[i] = 0xFFFFFFFFu;   // padding: no code's top digit exceeds 4
        if (rv && e < cr) k[i] = stg32[2 * CK_(pr + e, STAGE, 42) + 1] | e;
    }
    kpl_sort<K, W>(k);
#pragma unroll
    for (uint32_t i = 0; i < K; ++i) {
        const uint32_t e = K * l + i;
        if (rv && e < cr)
            a.sfids[CK_((uint64_t)dr + e, a.sfids_cap, 44)] =
                stg32[2 * CK_(pr + (k[i] & (W - 1)), STAGE, 43)] & (uint32_t)~KEY_MASK;
    }
}

// Tile epilogue: sort the 64 rows of this wave and write their filter ids to
// sfids[dst .. dst + c).  The rows are pulled into LDS a chunk of whole rows at
// a time (at most STAGE elements), eight rows per batch of independent loads:
// the rows were written moments ago but have usually left L2, so a dependent
// load per sort group would pay full memory latency ~20 times per tile.  Rows
// of size class W (W/2 < c <= W, W = 2..64) are then packed 64/W per
// wave-instruction, one element per lane, and sorted by a W-wide bitonic
// network of __shfl_xor exchanges.  65..128 elements: rank count, two per lane.
// `free` (wave-uniform): zero low bits of every staged code's high word; a
// class with log2(W) <= free takes the tagged u32 network above -- with
// TM_SORT_KPL keys per lane its own classes, 64 K / W rows per pass.
template <bool CK, class LT>
__device__ __forceinline__ void sort_classes(const MatchArgs& a, LT& L, bool keep, uint32_t c, uint32_t pos,
                                             uint32_t dst, uint32_t free) {
    constexpr uint32_t STAGE = LT::STAGE;
    uint32_t lane = threadIdx.x;
#if TM_SORT_KPL > 1
    // an empty asm re-defines the lane id here: every class derives a few
    // values from it alone (its place in a row, its row in a pass), and as
    // loop invariants of the wave's tile loop they were all hoisted out of it
    // and held in VGPRs through the whole kernel (128 VGPRs and 18 spilled
    // with both sets of classes; 104 with this line)
    asm volatile("" : "+v"(lane));
#endif
    const unsigned long long* stg = reinterpret_cast<const unsigned long long*>(L.q);
    if (keep && c == 1) a.sfids[CK_(dst, a.sfids_cap, 40)] = (uint32_t)(stg[CK_(pos, STAGE, 41)] & ~KEY_MASK);
    uint32_t upto = 1;   // rows of up to this many entries are done (wave-uniform)
#if TM_SORT_KPL > 1
    // Tagged classes, K = TM_SORT_KPL keys per lane, while log2(W) <= free:
    // rows of 2..K entries sort inside their own lane (no list, no shuffle, no
    // barrier: the row's lane is the owner), rows of K + 1..4 K share a class
    // of four lanes, then W = 8 K .. 128 at W / K lanes a row.  What is left
    // (free too small for a class, or none at all) takes the loops below as
    // before.
    if (TM_TAGGED_SORT) {
        constexpr uint32_t K = TM_SORT_KPL;
        const uint32_t* stg32 = reinterpret_cast<const uint32_t*>(L.q);
        if ((K >> free) <= 1) {
            const bool mine = keep && c > 1 && c <= K;
            if (__ballot(mine)) kpl_pass<CK, K, K, STAGE>(a, stg32, mine, 0u, c, pos, dst);
            upto = K;
        }
#pragma unroll
        for (uint32_t W = 4 * K; W <= 128; W <<= 1) {
            if ((W >> free) > 1) break;   // log2(W) > free: this class and the wider ones sort u64
            const bool mine = keep && c > (W == 4 * K ? K : W / 2) && c <= W;
            upto = W;
            const uint64_t m = __ballot(mine);
            if (!m) continue;
            const uint32_t nrows = __popcll(m);
            if (mine) L.list[prefix_count(m)] = lane;
            __syncthreads();
            const uint32_t LPR = W / K, STEP = 64 / LPR;
            for (uint32_t g = 0; g < nrows; g += STEP) {
                const uint32_t r = g + lane / LPR;
                const bool rv = r < nrows;
                const uint32_t owner = rv ? L.list[r] : 0u;
                const uint32_t cr = __shfl(c, owner, 64);
                const uint32_t pr = __shfl(pos, owner, 64);
                const uint32_t dr = __shfl(dst, owner, 64);
                const uint32_t l = lane & (LPR - 1);
                switch (W) {
                case 8: kpl_pass<CK, K, 8, STAGE>(a, stg32, rv, l, cr, pr, dr); break;
                case 16: kpl_pass<CK, K, 16, STAGE>(a, stg32, rv, l, cr, pr, dr); break;
                case 32: kpl_pass<CK, K, 32, STAGE>(a, stg32, rv, l, cr, pr, dr); break;
                case 64: kpl_pass<CK, K, 64, STAGE>(a, stg32, rv, l, cr, pr, dr); break;
                default: kpl_pass<CK, K, 128, STAGE>(a, stg32, rv, l, cr, pr, dr); break;
                }
            }
            __syncthreads();
        }
        if (!__ballot(keep && c > upto)) return;
    }
#endif
#pragma unroll
    for (uint32_t W = 2; W <= 64; W <<= 1) {
        const bool mine = keep && c > upto && c > W / 2 && c <= W;
        const uint64_t m = __ballot(mine);
        if (!m) continue;
        const uint32_t nrows = __popcll(m);
        if (mine) L.list[prefix_count(m)] = lane;
        __syncthreads();
        const uint32_t e = lane & (W - 1);
        const uint32_t STEP = 64 / W;
        for (uint32_t g = 0; g < nrows; g += STEP) {
            const uint32_t r = g + lane / W;
            const bool rv = r < nrows;
            const uint32_t owner = rv ? L.list[r] : 0u;
            const uint32_t cr = __shfl(c, owner, 64);
            const uint32_t pr = __shfl(pos, owner, 64);
            const uint32_t dr = __shfl(dst, owner, 64);
            // log2(W) <= free (one key per lane only: with more, the classes
            // above take the tagged rows and what reaches this loop sorts u64)
            if (TM_TAGGED_SORT && TM_SORT_KPL == 1 && (W >> free) <= 1) {
                const uint32_t* stg32 = reinterpret_cast<const uint32_t*>(L.q);
                uint32_t k32 = 0xFFFFFFFFu;   // padding: no code's top digit exceeds 4
                if (rv && e < cr) k32 = stg32[2 * CK_(pr + e, STAGE, 42) + 1] | e;
                switch (W) {
                case 2: k32 = tag_sort<2>(k32); break;
                case 4: k32 = tag_sort<4>(k32); break;
                case 8: k32 = tag_sort<8>(k32); break;
                case 16: k32 = tag_sort<16>(k32); break;
                case 32: k32 = tag_sort<32>(k32); break;
                default: k32 = tag_sort<64>(k32); break;
                }
                // sorted place e holds the entry that arrived as number k32 & (W - 1)
                if (rv && e < cr)
                    a.sfids[CK_((uint64_t)dr + e, a.sfids_cap, 44)] =
                        stg32[2 * CK_(pr + (k32 & (W - 1)), STAGE, 43)] & (uint32_t)~KEY_MASK;
                continue;
            }
            unsigned long long key = ~0ull;
            if (rv && e < cr) key = stg[CK_(pr + e, STAGE, 42)];
#pragma unroll
            for (uint32_t kk = 2; kk <= W; kk <<= 1) {
#pragma unroll
                for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
                    const unsigned long long other = xor_lane64(key, j);
                    const bool up = (e & kk) == 0;
                    const bool lower = (e & j) == 0;
                    const unsigned long long lo = key < other ? key : other;
                    const unsigned long long hi = key < other ? other : key;
                    key = (lower == up) ? lo : hi;
                }
            }
            if (rv && e < cr) a.sfids[CK_((uint64_t)dr + e, a.sfids_cap, 44)] = (uint32_t)(key & ~KEY_MASK);
        }
        __syncthreads();
    }
    {
        const bool mine = keep && c > 64 && c > upto;
        uint64_t m = __ballot(mine);
        while (m) {
            const uint32_t owner = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t cr = __shfl(c, owner, 64);
            const uint32_t pr = __shfl(pos, owner, 64);
            const uint32_t dr = __shfl(dst, owner, 64);
            unsigned long long k0 = ~0ull, k1 = ~0ull;
            if (lane < cr) k0 = stg[CK_(pr + lane, STAGE, 45)];
            if (lane + 64 < cr) k1 = stg[CK_(pr + lane + 64, STAGE, 46)];
            uint32_t r0 = 0, r1 = 0;
            for (uint32_t j = 0; j < 64; ++j) {
                const unsigned long long kj = __shfl(k0, j, 64);
                r0 += kj < k0 ? 1u : 0u;
                r1 += kj < k1 ? 1u : 0u;
            }
            for (uint32_t j = 64; j < cr; ++j) {
                const unsigned long long kj = __shfl(k1, j - 64, 64);
                r0 += kj < k0 ? 1u : 0u;
                r1 += kj < k1 ? 1u : 0u;
            }
            if (lane < cr) a.sfids[CK_((uint64_t)dr + r0, a.sfids_cap, 47)] = (uint32_t)(k0 & ~KEY_MASK);
            if (lane + 64 < cr) a.sfids[CK_((uint64_t)dr + r1, a.sfids_cap, 48)] = (uint32_t)(k1 & ~KEY_MASK);
        }
    }
}

#ifndef TM_PREFETCH_NEXT
#define TM_PREFETCH_NEXT 2   // 0: a tile's prologue loads its own offsets, flags and words; 1: offsets and flags ahead; 2: the words too
#endif
// Next-tile prefetch.  A tile's prologue used to pay two memory latencies in
// a row (toff[] / tflags[], then the words they locate) for addresses known a
// tile earlier.  The wave now loads them into registers while the previous
// tile's epilogue runs: the per-lane offsets and flags right after the
// frontier loop, the words once the read-back's first wait has brought the
// offsets in.  The next prologue writes LDS from the registers.
struct TileAhead {
    uint32_t off, end, fl;    // toff[t], toff[t + 1], tflags[t] of this lane's topic (0, 0, TF_SLOW: no topic)
#if TM_PREFETCH_NEXT >= 2
    uint32_t w[WCAP / 64];    // words wbeg + lane + 64 j of a tile whose words fit the LDS cache
#endif
};

template <bool CK>
__device__ __forceinline__ void ahead_meta(const MatchArgs& a, uint32_t tile, uint32_t tt, TileAhead& p) {
    const uint32_t lane = threadIdx.x;
    const uint32_t t = tile * tt + lane;
    p.off = 0; p.end = 0; p.fl = TF_SLOW;
    if (lane < tt && t < a.n) {
        p.off = a.toff[CK_(t, a.n + 1, 4)];
        p.end = a.toff[CK_(t + 1, a.n + 1, 5)];
        p.fl = a.tflags[CK_(t, a.n, 6)];
    }
}

// the tile's word range, from the lanes of its first and last topic (tile < ntiles: lane 0 has a topic)
__device__ __forceinline__ void ahead_range(const MatchArgs& a, uint32_t tile, uint32_t tt, const TileAhead& p,
                                            uint32_t& wbeg, uint32_t& wend) {
    const uint32_t nv = min(tt, a.n - tile * tt);
    wbeg = __builtin_amdgcn_readlane(p.off, 0);
    wend = __builtin_amdgcn_readlane(p.end, nv - 1);
}

template <bool CK>
__device__ __forceinline__ void ahead_words(const MatchArgs& a, uint32_t tile, uint32_t tt, TileAhead& p) {
#if TM_PREFETCH_NEXT >= 2
    const uint32_t lane = threadIdx.x;
    uint32_t wbeg, wend;
    ahead_range(a, tile, tt, p, wbeg, wend);
    const uint32_t nw = wend - wbeg;
    if (nw > (uint32_t)WCAP) return;   // read from HBM by the walk itself
#pragma unroll
    for (uint32_t j = 0; j < WCAP / 64; ++j) {
        const uint32_t i = lane + 64 * j;
        if (i < nw) p.w[j] = a.words[CK_(wbeg + i, a.nwords, 8)];
    }
#endif
}

#ifndef TM_LOG_U
#define TM_LOG_U 12  // log entries per lane per read-back step, all in flight (4 / 8 / 12 / 16: 5.10 / 5.07 / 5.04 / 5.05 ms)
#endif
// Emission log epilogue: the tile's matches were appended
// to a wave-private log in iteration order (coalesced: one store of <= 64
// consecutive entries per emission role per iteration), each with its topic
// lane in a parallel byte log.  The rows are rebuilt in LDS a chunk of whole
// rows at a time -- the log is streamed (from memory, not from L2: a C2 wave's
// log is long gone from its XCD's 4 MiB by the time the tile's frontier is
// empty, the bucket reads of every wave having passed through it since) and
// every entry of a chunk's rows goes to its row's next free place -- and
// sorted as before.  ah_words: the next tile's word loads (TM_PREFETCH_NEXT),
// issued after the first chunk's read-back.
template <bool CK, class LT, class AW>
__device__ __forceinline__ void sort_rows_log(const MatchArgs& a, LT& L, bool keep, uint32_t c, uint32_t dst,
                                              unsigned long long* wlog, uint8_t* wlane, uint32_t lcount,
                                              PhaseClk& pc, const AW& ah_words) {
    constexpr uint32_t STAGE = LT::STAGE;
    const uint32_t lane = threadIdx.x;
    unsigned long long* stg = reinterpret_cast<unsigned long long*>(L.q);
    const uint32_t cw = keep ? c : 0u;
    uint32_t incl = cw;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += u;
    }
    const uint32_t pos = incl - cw;
    uint32_t rs = 0;
    while (rs < a.tile_topics) {
        const uint32_t p0 = __builtin_amdgcn_readlane(pos, rs);
        const uint64_t beyond = __ballot(lane >= rs && pos + cw - p0 > STAGE);
        const uint32_t re = beyond ? (uint32_t)__builtin_ctzll(beyond) : a.tile_topics;
        const bool in_chunk = keep && lane >= rs && lane < re;
        // (depth / toff are free after the frontier loop) row base in the
        // stage, NONE for rows not staged in this pass
        L.depth[lane] = in_chunk ? pos - p0 : NONE;
        L.toff[lane] = 0;                            // row fill cursor
        __syncthreads();
        uint32_t kor = 0;   // OR of the placed entries' code bits 31..62
        for (uint32_t k0 = 0; k0 < lcount; k0 += 64 * TM_LOG_U) {
            unsigned long long e[TM_LOG_U];
            uint32_t r[TM_LOG_U];
#pragma unroll
            for (uint32_t u = 0; u < TM_LOG_U; ++u) {
                const uint32_t k = k0 + lane + 64 * u;
                r[u] = 64;
                if (k < lcount) {
                    e[u] = wlog[k];
                    r[u] = wlane[k];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < TM_LOG_U; ++u) {
                const uint32_t base = r[u] < 64 ? L.depth[r[u]] : NONE;
                if (base == NONE) continue;
                const uint32_t at = base + atomicAdd(&L.toff[r[u]], 1u);
                stg[CK_(at, STAGE, 49)] = e[u];
                kor |= (uint32_t)(e[u] >> 31);
            }
        }
        // free low bits of the chunk's code high words: tz = ctz of the OR of
        // the codes, free = clamp(tz - 32, 0, 8) (bit 31, the level-10 digit's
        // lowest, is part of the code: set anywhere -> 0)
        uint32_t free = 0;
        if (TM_TAGGED_SORT) {
#pragma unroll
            for (uint32_t j = 1; j < 64; j <<= 1) kor |= xor_lane32(kor, j);
            const uint32_t tz = (uint32_t)__builtin_ctz(__builtin_amdgcn_readfirstlane(kor) | 0x200u);   // 0..9
            free = tz ? tz - 1 : 0u;
        }
        __syncthreads();
        pc.lap(PH_READBACK);
        // every load so far has come in, the next tile's offsets with them:
        // its words go out here, under the sort
        if (rs == 0) ah_words();
        sort_classes<CK, LT>(a, L, in_chunk, c, pos - p0, dst, free);
        __syncthreads();
        pc.lap(PH_SORT);
        rs = re;
    }
}

template <bool CK>
__device__ __forceinline__ void send_to_slow(const MatchArgs& a, bool mine, uint32_t t) {
    const uint64_t m = __ballot(mine);
    uint32_t base = 0;
    if (threadIdx.x == 0 && m) base = atomicAdd(&a.ctrl[CTRL_NOVF], (uint32_t)__popcll(m));
    base = __shfl(base, 0, 64);
    if (mine) {
        const uint32_t slot = base + prefix_count(m);
        if (slot < a.ovf_cap) a.ovf_list[CK_(slot, a.ovf_cap, 12)] = t;
        else atomicOr(&a.ctrl[CTRL_ERR], ERR_OVF_LIST);
    }
}

// One tile.  IN_LDS: the tile's words are staged in LDS (the common case);
// otherwise they are read from HBM.  Templated so word reads are plain ds_read
// or global_load, never flat.
// ah_meta / ah_words issue the next tile's loads (TM_PREFETCH_NEXT): each is
// called exactly once on every way out, ah_meta first.
template <bool CK, bool BIG, bool IN_LDS, class LT, class AM, class AW>
__device__ __forceinline__ void match_tile(const MatchArgs& a, LT& L, uint32_t t0, uint32_t tend, uint32_t wbase,
                                           uint8_t fl, bool valid, unsigned long long& sV, unsigned long long& sH,
                                           unsigned long long& sW, unsigned long long& sM, unsigned long long& sP,
                                           PhaseClk& pc, const AM& ah_meta, const AW& ah_words) {
    const uint32_t lane = threadIdx.x;
    const uint32_t t = t0 + lane;
    const uint32_t* wsrc = IN_LDS ? L.words : a.words;
    const uint32_t wlim = IN_LDS ? (uint32_t)WCAP : a.nwords;
    (void)wbase;

    uint32_t qn = 0;
    const bool active = !(fl & TF_SLOW);
    unsigned long long* const wrows = a.rows + (uint64_t)blockIdx.x * a.tile_topics * a.row_cap;
    // the wave's emission log: its rows region (entries) + a byte per entry
    // (topic lane) past the whole rows array
    const uint32_t lcap = a.tile_topics * a.row_cap;
    uint8_t* const wlane =
        reinterpret_cast<uint8_t*>(a.rows + (uint64_t)a.grid * lcap) + (uint64_t)blockIdx.x * lcap;
    uint32_t lcount = 0;
    uint32_t tV = 0, tH = 0, tP = 0;   // committed only if the tile does not overflow
    const uint32_t d_me = L.depth[lane];

    // ---- level 0: root expansion, one topic per lane
    {
        Expand x; x.ne = 0; x.np = 0;
        uint32_t w0 = 0;
        if (active && d_me > 0) {
            const bool dollar = fl & TF_DOLLAR;
            tV += 1;
            if (!dollar && (a.root.flags & NF_HASH)) tH += 1;
            w0 = wsrc[CK_(L.toff[lane], wlim, 9)];
            expand_root(a.root, dollar, d_me, w0, x);
        }
        const uint64_t b0 = __ballot(x.np >= 1), b1 = __ballot(x.np >= 2);
        const uint32_t pre = prefix_count(b0) + prefix_count(b1);
        const uint32_t meta = lane | (1u << M_LVL_SHIFT);
        const uint32_t wid = w0 & WID_MASK;
        if (x.np >= 1) L.q[qn + pre] = q_pack(x.pk0, meta | x.pf0, ROOT, (x.pf0 & M_PLUS) ? W_PLUS : wid);
        if (x.np >= 2) L.q[qn + pre + 1] = q_pack(x.pk1, meta | x.pf1, ROOT, (x.pf1 & M_PLUS) ? W_PLUS : wid);
        qn += __popcll(b0) + __popcll(b1);
        const uint64_t mr = __ballot(x.ne != 0);
        if (x.ne) {   // at most one emission at the root ('#')
            L.cnt[lane] = 1;
            const uint32_t i = prefix_count(mr);
            wrows[i] = (x.ek0 & KEY_MASK) | x.ef0;
            wlane[i] = (uint8_t)lane;
        }
        lcount = (uint32_t)__popcll(mr);
    }

    // ---- frontier loop: LIFO stack, up to 64 probes per iteration
    //
    // Quad-cooperative probing: probe p (0..63) of an iteration is read by the
    // quad of lanes 4q..4q+3 in round r, each lane loading one 16-B slot of
    // the 64-B bucket, so a load instruction touches 16 cache lines instead of
    // 64 (one L1 tag lookup per probe instead of four: the lookups, not the
    // bytes, saturate the L1 at full occupancy).  p = 4q + r: a probe's owner
    // lane p sits in the quad that reads its bucket, and the quad takes the
    // bucket, the parent and the word from its lane r by DPP quad_perm moves,
    // with no LDS round trip between the hash and the bucket loads.  The
    // popped entries stay in their LDS slots during the probe, and the quad
    // reports through the owner's entry: the lane whose slot matches stores the
    // slot over it whole, the lane of the bucket's last slot that slot's raw
    // parent field into the word field.  A key that spilled past its home
    // bucket is pushed again as a continuation (displacement + 1) rather than
    // holding the whole wave for a dependent read.
    // (TM_QUAD_OWN = 0: p = 16r + q, and the owner's bucket index goes through
    // its entry as well.)
    const uint32_t qd = lane >> 2, qs = lane & 3;
    // the entry of the probe that this lane's quad serves in round r
    const auto q_of = [&](uint32_t r) -> uint32_t { return TM_QUAD_OWN ? 4 * qd + r : 16 * r + qd; };
    // The loop's wave-uniform operands get scalar registers of their own (the
    // empty asm defines them anew): as parts of the kernel-argument tuples
    // they were spilled to VGPR lanes with the tuples' cold parts and read
    // back by v_readlane in every iteration.
    uint32_t nbk = a.nbuckets, maxp = a.max_probe, rcap = a.row_cap, nrec = BIG ? 0u : a.nslots * 16u;
    Slot* sbase = const_cast<Slot*>(a.slots);
    asm volatile("" : "+s"(nbk), "+s"(maxp), "+s"(rcap), "+s"(nrec), "+s"(sbase));
    // (a pointer that passes through the asm is generic: the loop reads the
    // table and HBM words through global pointers made from the integers)
    uint64_t wbits = IN_LDS ? 0ull : (uint64_t)a.words;
    if constexpr (!IN_LDS) asm volatile("" : "+s"(wbits));
    typedef const __attribute__((address_space(1))) uint32_t* gwords_t;
    typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) u32x4_t* gslots_t;
    const auto word_at = [&](uint64_t i) -> uint32_t { return IN_LDS ? L.words[i] : ((gwords_t)wbits)[i]; };
    pc.lap(PH_PROLOGUE);
    while (qn > 0) {
        const uint32_t k = min(qn, 64u);
        const bool has = lane < k;
        qn -= k;
        // bucket reads (hits, misses, continuations) | iterations << 20: the same
        // in every lane; kept in a VGPR (as a scalar it is spilled to a lane
        // and reloaded every iteration)
        tP += k + (1u << 20);
        asm volatile("" : "+v"(tP));
        // A lane without a probe of its own (k < 64, the stack's last pop)
        // takes lane 0's entry along: every index derived from it (topic
        // lane, word offsets, row count) is then a live one, so the reads
        // below need no exec region of their own and `has` only gates what a
        // lane pushes, emits and counts.
        const uint32_t idx = qn + (has ? lane : 0u);
        const uint4 e = L.q[idx];
        const uint32_t meta = e.x & 0x7FFFFFFFu;
        const uint64_t key = ((uint64_t)e.y << 32) | (e.x & 0x80000000u);
        const uint32_t parent = e.z, pw = e.w;
        const uint32_t tl = meta & 63;
        const uint32_t lc = (meta >> M_LVL_SHIFT) & M_LVL_MASK;
        const uint32_t disp = (meta >> M_DISP_SHIFT) & M_DISP_MASK;
        uint32_t hb = home_bucket(parent, pw, nbk) + disp;
        if (hb >= nbk) hb -= nbk;
#if TM_QUAD_OWN
        // What the owner offers its quad.  A lane without a probe offers a
        // parent that no masked parent field equals, and a bucket that is
        // safe to read: past the descriptor's range (reads 0, no memory
        // access), or bucket 0 where the table is read with plain loads.  So
        // the rounds need no validity test of their own.
        if (CK) hb = (uint32_t)(CK_((uint64_t)hb * BUCKET + (BUCKET - 1), a.nslots, 1) / BUCKET);
        const uint32_t o_par = has ? parent : SLOT_EMPTY;
        const uint32_t o_bkt = BIG ? (has ? hb : 0u) : (has ? hb * (uint32_t)(BUCKET * sizeof(Slot)) : OFF_NONE);
#else
        L.q[idx].x = hb;   // (a lane without a probe repeats lane 0's value at lane 0's address)
#endif
        // the slot table's descriptor, put together here from its scalars (the
        // asm keeps it from being hoisted: as a loop-invariant 4-dword tuple it
        // was spilled and read back lane by lane, with a hazard pad, every time)
        asm volatile("" : "+s"(sbase), "+s"(nrec));
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(sbase, 0, nrec, 0x00020000);
        uint32_t rp[4], rw[4];
        uint4 sl[4];
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
#if TM_QUAD_OWN
            rp[r] = quad_bcast(o_par, r);
            rw[r] = quad_bcast(pw, r);
            const uint32_t ob = quad_bcast(o_bkt, r);
            if (!BIG) {
                sl[r] = ld_b128(rsrc, ob + qs * (uint32_t)sizeof(Slot));
            } else {
                const u32x4_t g = ((gslots_t)(uint64_t)sbase)[(uint64_t)ob * BUCKET + qs];
                sl[r] = uint4{g[0], g[1], g[2], g[3]};
            }
#else
            const uint32_t p = q_of(r);
            const bool v = p < k;
            const uint4 rec = L.q[qn + (v ? p : 0u)];
            rp[r] = v ? rec.z : SLOT_EMPTY;
            rw[r] = rec.w;
            const uint64_t si = CK_((uint64_t)rec.x * BUCKET + qs, a.nslots, 1);
            if (!BIG) {
                sl[r] = ld_b128(rsrc, v ? (uint32_t)si * 16u : 0xFFFFFFF0u);   // out of range: reads 0
            } else {
                const u32x4_t g = v ? ((gslots_t)(uint64_t)sbase)[si] : u32x4_t{0u, 0u, 0u, 0u};
                sl[r] = uint4{g[0], g[1], g[2], g[3]};
            }
#endif
        }
        // the topic's words are read while the buckets are in flight (the
        // barrier keeps the compiler from hoisting these LDS reads, and their
        // waits, above the bucket loads)
        __builtin_amdgcn_sched_barrier(0);
        // (every pushed entry has 1 <= lc <= d: a push raises lc only below
        // the end of the words)  At the end of the words w_here repeats
        // w_prev; nothing that is used there reads it.
        const uint32_t base = L.toff[tl];
        const uint32_t d = L.depth[tl];
        const bool at_end = lc == d;
        const uint32_t w_here = word_at(CK_(base + lc - (at_end ? 1u : 0u), wlim, 11));
        const uint32_t w_prev = word_at(CK_(base + lc - 1, wlim, 10));
        // The quad reports to the owner through the owner's LDS entry, not
        // through ballots.  (rp is SLOT_EMPTY where the quad has no probe,
        // which no masked parent field equals.)
        uint32_t qs_now = qs;   // (compared here: the hoisted lane mask would be one more spilled pair)
        asm volatile("" : "+v"(qs_now));
#if TM_QUAD_OWN == 1
        // The last slot's lane stores its slot's raw parent field into the
        // word field of every round's entry, under one exec region for the
        // four: SLOT_EMPTY there says that the probe run ends in this bucket.
        // A quad without a probe (out-of-range load: reads 0) writes above the
        // popped entries: when k < 64, qn is 0 after the pop and qn + p < 64
        // is unused stack; when k = 64 every quad has a probe.
        if (qs_now == 3) {
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) L.q[qn + q_of(r)].w = sl[r].x;
        }
        // Then the matching lane stores its slot over the entry, whole: a slot
        // has the entry's shape, and the owner reads everything it needs off
        // the slot's own fields.  A wave's LDS operations complete in order,
        // so a match in the last slot overwrites that probe's tail word.
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const bool m = (sl[r].x & ID_MASK) == rp[r] && (sl[r].y & WID_MASK) == rw[r];
            if (m) L.q[qn + q_of(r)] = sl[r];
        }
        const uint4 res = L.q[idx];
        // a row already longer than K goes to the generic path whole: its
        // entries are not expanded further (C5 K = 1000: ~10k rows of ~1,000
        // matches each stopped at K + 1 instead of walked to the end)
        const bool live = has & (L.cnt[tl] <= rcap);
        // An entry that still holds its parent was not found: a found one
        // holds the slot's child field, and a child's id is never its parent's
        // (new_node takes a free or a fresh id while the parent is live, ROOT
        // is nobody's child; the flag bits lie above the 30-bit id).
        const bool found = live & (res.z != parent);
        const bool cont = live & !found & (res.w != SLOT_EMPTY) & (disp < maxp);
        // the found child's summary (the slot's child and hash fields) and its
        // literal signature (the top bits of the slot's key fields)
        const uint32_t hz = res.z, hw = res.w;
        const uint32_t lsig = slot_lsig(res.x, res.y);
#else
        // The matching lane writes the child summary and a FOUND mark, the
        // lane of the bucket's last slot a TAIL mark when that slot is free
        // (the probe run ends in this bucket).  Parent ids and word ids never
        // equal the marks.
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const bool m = (sl[r].x & ID_MASK) == rp[r] && (sl[r].y & WID_MASK) == rw[r];
            if (m) {
                L.q[qn + q_of(r)].x = sl[r].z;
                L.q[qn + q_of(r)].y = sl[r].w;
                L.q[qn + q_of(r)].z = Q_FOUND | slot_lsig(sl[r].x, sl[r].y);
            }
        }
        // The last slot's lane writes the word field in every round, under one
        // exec region for the four: TAIL, or the word it read from there.  A
        // quad without a probe (out-of-range load: reads 0) puts entry qn's
        // word into a place above the popped ones: when k < 64, qn is 0 after
        // the pop and qn + p < 64 is unused stack; when k = 64 every quad has
        // a probe.
        if (qs_now == 3) {
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r) L.q[qn + q_of(r)].w = sl[r].x == SLOT_EMPTY ? Q_TAIL : rw[r];
        }
        const uint4 res = L.q[idx];
        // a row already longer than K goes to the generic path whole: its
        // entries are not expanded further (C5 K = 1000: ~10k rows of ~1,000
        // matches each stopped at K + 1 instead of walked to the end)
        const bool live = has & (L.cnt[tl] <= rcap);
        const bool found = live & (res.z >= Q_FOUND);
        const bool cont = live & !found & (res.w != Q_TAIL) & (disp < maxp);
        // the found child's summary (bits of the slot's child and hash fields)
        const uint32_t hz = res.x, hw = res.y;
        const uint32_t lsig = res.z;   // (the mark's bits lie above the signature's)
#endif
        const uint32_t child = hz & ID_MASK, hterm = hw & ID_MASK;
        const bool n_topic = (hz & B_TOPIC) != 0, n_plus = (hz & B_PLUS) != 0;
        const bool n_hterm = (hw & B_HTERM) != 0, n_hash = (hw & B_HASH) != 0;
        // Expansion of the found node, match_node/3 (src/emqx_trie.erl:168-177),
        // with fixed roles instead of expand()'s packed lists: emissions A, B;
        // push L (the literal word, or the continuation) and push P ('+').
        // lc <= FAST_MAX_DEPTH here, so every level has a digit position.
        // Straight-line: both arms are computed and selected (non-short-circuit
        // & and |), since an exec region costs more than the few VALU it skips.
        const uint32_t cls = w_here >> WID_BITS, id = w_here & WID_MASK;
        const int sh = key_shift(lc);
        tV += (found & !(meta & M_DSTART)) ? 1u : 0u;
        tH += (found & n_hash) ? 1u : 0u;
        // end of the words: own topic, then the '#' child's; otherwise the '#'
        // child's topic, then the literal and '+' edges
        const bool eA0 = found & (at_end ? (!(meta & M_SKIPE) & n_topic) : n_hterm);
        const bool eB0 = found & at_end & n_hterm;
        const uint32_t fA = at_end ? child : hterm;
        // '' word at level lc-1 followed by the end: "P/" sorts before "P/#"
        // (digit 4 -> 1 at that level)
        const int sp = sh + 3;   // key_shift(lc - 1)
        const bool redigit = ((w_prev >> WID_BITS) == C_EMPTY) & (((key >> sp) & 7) == 4);
        // one shift for both arms: level lc's digit bits are still zero in
        // key, so or-ing the '#' digit in is an xor as well
        const uint64_t kA = key ^ ((uint64_t)(at_end ? (redigit ? 5u : 0u) : dig_H(cls)) << (at_end ? sp : sh));
        // a literal word whose signature bit is clear has no edge here
        // (and, for a node without a '#' child, its 30-bit signature)
        const bool lit = (id != W_UNKNOWN) & (id != W_PLUS) & (((lsig >> lsig_pos(id)) & 1u) != 0) &
                         (n_hash | (((hw >> lext_pos(id)) & 1u) != 0));
        const bool pL = found & !at_end & (id == W_HASH ? n_hash : lit);
        const bool pP = found & !at_end & n_plus;
        bool eA = eA0, eB = eB0;
        const bool sL = cont | pL;
        const uint64_t bL = __ballot(sL), bP = __ballot(pP);
        const uint32_t ptot = __popcll(bL) + __popcll(bP);
        if (qn + ptot > (uint32_t)LT::QCAP) break;   // stack overflow: leaves qn > 0 (ptot <= 128 < QCAP)
        const uint32_t pre = qn + prefix_count(bL) + prefix_count(bP);
        const uint32_t nmeta = tl | ((lc + 1) << M_LVL_SHIFT);
        if (sL) {
            const uint32_t lfl = ((id == W_HASH) & (lc + 1 == d)) ? M_SKIPE : 0u;
            const uint64_t kL = cont ? key : key | ((uint64_t)dig_L(cls) << sh);
            L.q[pre] = q_pack(kL, cont ? meta + (1u << M_DISP_SHIFT) : nmeta | lfl, cont ? parent : child,
                              cont ? pw : id);
        }
        if (pP) L.q[pre + (sL ? 1u : 0u)] = q_pack(key | ((uint64_t)dig_P(cls) << sh), nmeta | M_PLUS, child, W_PLUS);
        qn += ptot;
        {
            // row sizes; a row's entries past K are not logged (the row goes to
            // the generic path), so the log holds at most tile_topics * K
            uint32_t slot = 0;
            if (eA | eB) slot = atomicAdd(&L.cnt[tl], (eA ? 1u : 0u) + (eB ? 1u : 0u));
            const uint32_t slotB = slot + (eA ? 1u : 0u);
            eA = eA && slot < rcap;
            eB = eB && slotB < rcap;
            const uint64_t mA = __ballot(eA), mB = __ballot(eB);
            const uint32_t nA = (uint32_t)__popcll(mA), nE = nA + (uint32_t)__popcll(mB);
            if (eA) {
                const uint32_t i = lcount + prefix_count(mA);
                wrows[CK_(i, lcap, 13)] = (kA & KEY_MASK) | fA;
                wlane[i] = (uint8_t)tl;
            }
            if (eB) {
                const uint32_t i = lcount + nA + prefix_count(mB);
                wrows[CK_(i, lcap, 14)] = ((key | (2ull << sh)) & KEY_MASK) | hterm;
                wlane[i] = (uint8_t)tl;
            }
            lcount += nE;
        }
    }
    __syncthreads();
    pc.lap(PH_LOOP);
    ah_meta();

    if (qn > 0) {
        // probe stack overflow: every regular topic of the tile goes to the slow path
        send_to_slow<CK>(a, valid && active, t);
        ah_words();
        return;
    }
    // The wave's sums are wave-uniform (scalar registers): a tile's per-lane
    // counts are added up here, once per tile, rather than carried as five
    // u64 per lane through every tile and summed at the kernel's end.  (The
    // topic's word count is read again, not carried through the loop:
    // depth[] is intact until the read-back.)
    sV += tile_sum(tV); sH += tile_sum(tH);
    sW += tile_sum((active && L.depth[lane] > 0) ? L.depth[lane] : 0u);
    {
        const uint32_t p = __builtin_amdgcn_readfirstlane(tP);
        sP += (p & 0xFFFFFu) | ((unsigned long long)(p >> 20) << 40);   // probes | iterations << 40
    }
    const uint32_t c_me = L.cnt[lane];
    const bool row_ovf = valid && active && c_me > a.row_cap;   // row longer than K
    send_to_slow<CK>(a, row_ovf, t);
    const bool keep = valid && active && !row_ovf;
    const uint32_t c = keep ? c_me : 0u;
    // one contiguous staging run per tile: exclusive scan of the counts
    uint32_t incl = c;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += u;
    }
    const uint32_t tot = __shfl(incl, 63, 64);
    // u64 ticket: a batch may reserve more than 2^32 entries; the host then
    // fails it with TM_EOVERFLOW (sfids_cap < 2^32, so dst below never wraps)
    unsigned long long base64 = 0;
    const uint32_t g = (blockIdx.x % TICKET_GROUPS) & a.sgmask;   // my group's staging region
    if (lane == 0 && tot) base64 = atomicAdd(xg_top(a.xg, g), (unsigned long long)tot);
    base64 = __shfl(base64, 0, 64);
    const bool fits = base64 + tot <= a.rcap;
    base64 += (uint64_t)g * a.rcap;
    const uint32_t base = (uint32_t)base64;
    const uint32_t dst = base + incl - c;
    pc.lap(PH_SORT);   // the staging reservation counts as staging
    if (fits) {
        sort_rows_log<CK, LT>(a, L, keep, c, dst, wrows, wlane, lcount, pc, ah_words);
    } else {
        if (lane == 0) atomicOr(&a.ctrl[CTRL_ERR], ERR_STAGING);   // host grows sfids[] and reruns
        ah_words();
    }
    if (keep) {
        a.count[CK_(t, a.n, 16)] = c_me;
        a.src[CK_(t, a.n, 17)] = dst;
    }
    sM += __builtin_amdgcn_readfirstlane(tot);   // the kept rows' sizes
    pc.lap(PH_SORT);
    (void)tend;
}

#ifndef TM_DN_TILES_PER_WAVE
#define TM_DN_TILES_PER_WAVE 4
#endif
// device-counted batches: tiles shrink until each wave has this many to take
constexpr uint32_t DN_TILES_PER_WAVE = TM_DN_TILES_PER_WAVE;

template <bool CK, bool BIG, int QC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QC == 384 ? TM_WPE384 : 3, 8))) void tm_match_tiles(MatchArgs a) {
    __shared__ TileLds<QC> L;
    if (a.d_n) {
        // a device-deduplicated batch: its rows are counted on the device.
        // The grid was sized for the bound (every publish); tiles shrink
        // until the rows cover every wave (a C5 batch's ~186k rows would
        // otherwise be 2,900 tiles for 4,096 waves, the hot ones long)
        a.n = *a.d_n;
        while (a.tile_topics > 1 && (a.n + a.tile_topics - 1) / a.tile_topics < DN_TILES_PER_WAVE * gridDim.x)
            a.tile_topics >>= 1;
        // the host sized the static share for every publish: the rows take
        // half of their own tiles round-robin, the rest by tickets (a skewed
        // batch's hot rows come first, in the first tiles)
        const uint32_t nt = (a.n + a.tile_topics - 1) / a.tile_topics;
        a.static_rounds = max(1u, nt / (2u * gridDim.x));
    }
    const uint32_t lane = threadIdx.x;
    const uint32_t tt = a.tile_topics;   // topics per tile: 64, or fewer for small batches
    const uint32_t ntiles = (a.n + tt - 1) / tt;
    unsigned long long sV = 0, sH = 0, sW = 0, sM = 0, sP = 0;
    PhaseClk pc;

    // static round-robin tiles, then tickets for the tail; a ticket is taken at
    // the start of a tile so its latency hides behind the tile's work
    uint32_t tile = blockIdx.x, round = 0;
#if TM_PREFETCH_NEXT
    TileAhead nx;
    if (tile < ntiles) {   // the wave's first tile has nothing to hide behind
        ahead_meta<CK>(a, tile, tt, nx);
        ahead_words<CK>(a, tile, tt, nx);
    }
#endif
    while (tile < ntiles) {
        // the next tile: round-robin for the first static_rounds, then from a
        // ticket (a contended counter's latency would stall every in-order vmcnt
        // wait of the tile, so only the tail balances by tickets, per XCD)
        pc.start();
        uint32_t ticket = 0;
        if (round + 1 >= a.static_rounds && lane == 0)
            ticket = atomicAdd(&a.xg[(blockIdx.x % TICKET_GROUPS) * TICKET_STRIDE], 1u);
        const uint32_t t0 = tile * tt;
        const uint32_t tend = min(t0 + tt, a.n);
        const uint32_t t = t0 + lane;
        const bool valid = lane < tt && t < a.n;
#if TM_PREFETCH_NEXT
        // this tile's inputs are in nx, loaded under the previous tile's epilogue
        uint32_t wbeg, wend;
        ahead_range(a, tile, tt, nx, wbeg, wend);
        const bool in_lds = (wend - wbeg) <= (uint32_t)WCAP;
        const uint32_t my_off = valid ? nx.off : wend;
        const uint32_t my_end = valid ? nx.end : wend;
        const uint8_t fl = (uint8_t)nx.fl;
#if TM_PREFETCH_NEXT >= 2
        if (in_lds) {
#pragma unroll
            for (uint32_t j = 0; j < WCAP / 64; ++j) {
                const uint32_t i = lane + 64 * j;
                if (i < wend - wbeg) L.words[CK_(i, WCAP, 7)] = nx.w[j];
            }
        }
#else
        if (in_lds)
            for (uint32_t i = lane; i < wend - wbeg; i += 64) L.words[CK_(i, WCAP, 7)] = a.words[CK_(wbeg + i, a.nwords, 8)];
#endif
#else
        const uint32_t wbeg = a.toff[CK_(t0, a.n + 1, 2)], wend = a.toff[CK_(tend, a.n + 1, 3)];
        const bool in_lds = (wend - wbeg) <= (uint32_t)WCAP;
        const uint32_t my_off = valid ? a.toff[CK_(t, a.n + 1, 4)] : wend;
        const uint32_t my_end = valid ? a.toff[CK_(t + 1, a.n + 1, 5)] : wend;
        const uint8_t fl = valid ? a.tflags[CK_(t, a.n, 6)] : (uint8_t)TF_SLOW;
        if (in_lds)
            for (uint32_t i = lane; i < wend - wbeg; i += 64) L.words[CK_(i, WCAP, 7)] = a.words[CK_(wbeg + i, a.nwords, 8)];
#endif
        L.toff[lane] = in_lds ? my_off - wbeg : my_off;
        L.depth[lane] = my_end - my_off;
        L.cnt[lane] = 0;
        __syncthreads();
        // the tile after this one: round-robin, or the ticket taken above.  Its
        // loads are issued from inside match_tile, once the frontier is empty;
        // none when this is the wave's last tile.
        uint32_t next = ntiles;
        const auto next_tile = [&]() -> uint32_t {
            return round + 1 < a.static_rounds
                       ? blockIdx.x + (round + 1) * gridDim.x
                       : a.static_rounds * gridDim.x + __builtin_amdgcn_readfirstlane(ticket) * TICKET_GROUPS +
                             blockIdx.x % TICKET_GROUPS;
        };
#if TM_PREFETCH_NEXT
        const auto ah_meta = [&] {
            next = next_tile();
            if (next < ntiles) ahead_meta<CK>(a, next, tt, nx);
        };
        const auto ah_words = [&] {
            if (next < ntiles) ahead_words<CK>(a, next, tt, nx);
        };
#else
        const auto ah_meta = [&] { next = next_tile(); };
        const auto ah_words = [] {};
#endif
        if (in_lds) match_tile<CK, BIG, true>(a, L, t0, tend, wbeg, fl, valid, sV, sH, sW, sM, sP, pc, ah_meta, ah_words);
        else match_tile<CK, BIG, false>(a, L, t0, tend, wbeg, fl, valid, sV, sH, sW, sM, sP, pc, ah_meta, ah_words);
        __syncthreads();
        ++round;
        tile = next;
    }

    if (lane == 0 && a.wstats) {
        // the wave's sums, added up by tm_stats_reduce: ~4,000 waves ending
        // together would queue 6 same-line device atomics each (~30 ns apiece)
        unsigned long long* w = a.wstats + (uint64_t)blockIdx.x * WSTATS;
        w[0] = sV; w[1] = sH; w[2] = sW; w[3] = sM;
        w[4] = sP & ((1ull << 40) - 1); w[5] = sP >> 40;
#if TM_PHASE_CYCLES
        for (uint32_t k = 0; k < PHASE_N; ++k) w[6 + k] = pc.sum[k];
#endif
    } else if (lane == 0) {
        atomicAdd(&a.stats[ST_VISITS], sV); atomicAdd(&a.stats[ST_HASH], sH);
        atomicAdd(&a.stats[ST_WORDS], sW); atomicAdd(&a.stats[ST_MATCHES], sM);
        atomicAdd(&a.stats[ST_PROBES], sP & ((1ull << 40) - 1));
        atomicAdd(&a.stats[ST_ITERS], sP >> 40);
#if TM_PHASE_CYCLES
        for (uint32_t k = 0; k < PHASE_N; ++k) atomicAdd(&a.stats[ST_PHASE + k], pc.sum[k]);
#endif
    }
}

// the walk waves' sums -> the batch's stats (one block; after the walk)
__global__ __launch_bounds__(256) void tm_stats_reduce(const unsigned long long* w, uint32_t waves,
                                                       unsigned long long* stats) {
    constexpr uint32_t NS = 6 + PHASE_N;   // 6, or 10 with the phase cycle sums (TM_PHASE_CYCLES)
    __shared__ unsigned long long sh[4][NS];
    unsigned long long v[NS] = {};
    for (uint32_t i = threadIdx.x; i < waves; i += 256)
#pragma unroll
        for (uint32_t k = 0; k < NS; ++k) v[k] += w[(uint64_t)i * WSTATS + k];
#pragma unroll
    for (uint32_t k = 0; k < NS; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        const uint32_t k = threadIdx.x;
        const unsigned long long t = sh[0][k] + sh[1][k] + sh[2][k] + sh[3][k];
        const uint32_t idx[6] = {ST_VISITS, ST_HASH, ST_WORDS, ST_MATCHES, ST_PROBES, ST_ITERS};
        if (t) atomicAdd(&stats[k < 6 ? idx[k] : ST_PHASE + (k - 6)], t);
    }
}

// ---------------------------------------------------------------- slow path

// Erlang binary order on two filters (unsigned bytes, shorter prefix first).
template <bool CK>
__device__ __forceinline__ bool filter_less(const MatchArgs& a, uint32_t x, uint32_t y) {
    if (x == NONE) return false;
    if (y == NONE) return true;
    x = CK_(x, a.nnodes, 20); y = CK_(y, a.nnodes, 21);
    const uint8_t* px = a.fbytes + CK_(a.foff[x], a.nfbytes + 1, 22);
    const uint8_t* py = a.fbytes + CK_(a.foff[y], a.nfbytes + 1, 23);
    const uint32_t lx = a.flen[x], ly = a.flen[y];
    const uint32_t m = min(lx, ly);
    for (uint32_t i = 0; i < m; ++i)
        if (px[i] != py[i]) return px[i] < py[i];
    return lx < ly;
}

// Bitonic sort of n (power of two) (key, fid) pairs held at kp/fp (LDS or global).
template <bool CK>
__device__ void bitonic(const MatchArgs& a, unsigned long long* kp, uint32_t* fp, uint32_t n, bool by_bytes) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < n; i += 64) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const bool up = (i & k) == 0;
                    const bool gt = by_bytes ? filter_less<CK>(a, fp[ixj], fp[i]) : (kp[i] > kp[ixj]);
                    if (gt == up) {
                        const unsigned long long tk = kp[i]; kp[i] = kp[ixj]; kp[ixj] = tk;
                        const uint32_t tf = fp[i]; fp[i] = fp[ixj]; fp[ixj] = tf;
                    }
                }
            }
            __threadfence_block();
            __syncthreads();
        }
    }
}

// Generic path LDS: the probe stack while a topic is walked (SLOW_SQ 16-B
// entries {parent, meta, key lo, key hi}), then the same 8 KB as the row's
// sort area: 1,024 u64 (path code | filter id) or 2,048 u32 filter ids (rows
// ordered by bytes); a path-coded row of up to 2,048 sorts as two LDS runs
// merged on the way out (merge_runs_out).  A topic whose frontier outgrows the
// stack restarts in global scratch.  The walk is a chain of dependent probes
// per row, so the waves per CU set its pace: 8 KB of LDS per wave allows 20
// (16 KB: 10).
#ifndef TM_SLOW_SQ
#define TM_SLOW_SQ 512
#endif
constexpr uint32_t SLOW_SQ = TM_SLOW_SQ;
constexpr uint32_t SORT_LDS = SLOW_SQ * 2;    // u64 entries of the sort area
constexpr uint32_t SM_PLUS = 1u << 29;
constexpr uint32_t SM_SKIPE = 1u << 30;
constexpr uint32_t SM_DSTART = 1u << 31;
constexpr uint32_t SM_LVL = (1u << 29) - 1;

__device__ __forceinline__ uint32_t slow_flags(uint32_t pf) {
    return ((pf & M_PLUS) ? SM_PLUS : 0u) | ((pf & M_SKIPE) ? SM_SKIPE : 0u) | ((pf & M_DSTART) ? SM_DSTART : 0u);
}

// bitonic sort of n (power of two) u64 in LDS, ascending
__device__ void bitonic_lds64(unsigned long long* k, uint32_t n) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t kk = 2; kk <= n; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < n; i += 64) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const unsigned long long x = k[i], y = k[ixj];
                    if ((x > y) == ((i & kk) == 0)) { k[i] = y; k[ixj] = x; }
                }
            }
            __syncthreads();
        }
    }
}

// bitonic sort of n (power of two) filter ids in LDS by filter bytes
template <bool CK>
__device__ void bitonic_lds_bytes(const MatchArgs& a, uint32_t* f, uint32_t n) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t kk = 2; kk <= n; kk <<= 1) {
        for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
            for (uint32_t i = lane; i < n; i += 64) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint32_t x = f[i], y = f[ixj];
                    if (filter_less<CK>(a, y, x) == ((i & kk) == 0)) { f[i] = y; f[ixj] = x; }
                }
            }
            __syncthreads();
        }
    }
}

// A row of on (SORT_LDS < on <= 2 * SORT_LDS) path-coded entries whose first
// SORT_LDS, sorted, are back in okey[] (global scratch, as code | id) and the
// rest, sorted, in sk[0, nb) (LDS): every entry's place in the merged row is
// its index in its own run plus its rank in the other (a binary search: the
// keys are distinct, as a row's filter ids are), and its id goes there.
__device__ __forceinline__ void merge_runs_out(const unsigned long long* A, const unsigned long long* sk, uint32_t nb,
                                               uint32_t* out) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t i = lane; i < SORT_LDS; i += 64) {   // run A: rank in B (LDS)
        const unsigned long long x = A[i];
        uint32_t lo = 0, hi = nb;
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            if (sk[m] < x) lo = m + 1; else hi = m;
        }
        out[i + lo] = (uint32_t)(x & ~KEY_MASK);
    }
    for (uint32_t j = lane; j < nb; j += 64) {         // run B: rank in A (global)
        const unsigned long long x = sk[j];
        uint32_t lo = 0, hi = SORT_LDS;
        while (lo < hi) {
            const uint32_t m = (lo + hi) >> 1;
            if (A[m] < x) lo = m + 1; else hi = m;
        }
        out[j + lo] = (uint32_t)(x & ~KEY_MASK);
    }
}

template <bool CK, bool BIG>
__global__ __launch_bounds__(64) void tm_match_slow(MatchArgs a) {
    __shared__ uint4 sq[SLOW_SQ];
    unsigned long long* const sk = reinterpret_cast<unsigned long long*>(sq);   // (after the walk)
    uint32_t* const sfi = reinterpret_cast<uint32_t*>(sq);
    const uint32_t lane = threadIdx.x;
    const uint32_t wave = blockIdx.x;
    uint32_t* qpar = a.s_qparent + (size_t)wave * a.s_qcap;
    uint32_t* qmeta = a.s_qmeta + (size_t)wave * a.s_qcap;
    unsigned long long* qkey = a.s_qkey + (size_t)wave * a.s_qcap;
    uint32_t* ofid = a.s_ofid + (size_t)wave * a.s_ocap;
    unsigned long long* okey = a.s_okey + (size_t)wave * a.s_ocap;
    const uint32_t novf = min(a.ctrl[CTRL_NOVF], a.ovf_cap);
    const uint32_t n_slow = a.d_nslow ? min(*a.d_nslow, a.n) : a.n_slow;
    const uint32_t total_items = n_slow + novf;
    const uint32_t lcap = a.s_lcap && a.s_lcap < SLOW_SQ ? a.s_lcap : SLOW_SQ;
    unsigned long long sV = 0, sH = 0, sW = 0, sM = 0, sS = 0;

    for (uint32_t item = wave; item < total_items; item += gridDim.x) {
        uint32_t t = (item < n_slow) ? a.slow_list[CK_(item, n_slow, 24)]
                                     : a.ovf_list[CK_(item - n_slow, a.ovf_cap, 25)];
        t = CK_(t, a.n, 26);
        const uint8_t fl = a.tflags[t];
        const bool dollar = fl & TF_DOLLAR;
        const bool by_bytes = fl & TF_SLOW;   // deep or irregular: path code does not apply
        const uint32_t wb = a.toff[t];
        const uint32_t d = a.toff[t + 1] - wb;
        const uint32_t* w = a.words + wb;
        sS += 1;
        uint32_t qn = 0, on = 0;
        bool err = false;
        // the stack in LDS; a topic whose frontier outgrows it walks again
        // with the stack in its wave's global scratch (the counters of the
        // abandoned attempt are dropped)
        for (bool in_lds = true;;) {
            unsigned long long tV = 0, tH = 0, tW = 0;
            bool spill = false;
            qn = 0; on = 0;
            if (d > 0) {
                Expand x; x.ne = 0; x.np = 0;
                if (lane == 0) {
                    tV += 1; tW += d;
                    if (!dollar && (a.root.flags & NF_HASH)) tH += 1;
                    expand_root(a.root, dollar, d, w[0], x);
                    if (in_lds) {
                        if (x.np >= 1) sq[0] = uint4{ROOT, 1u | slow_flags(x.pf0), (uint32_t)x.pk0, (uint32_t)(x.pk0 >> 32)};
                        if (x.np >= 2) sq[1] = uint4{ROOT, 1u | slow_flags(x.pf1), (uint32_t)x.pk1, (uint32_t)(x.pk1 >> 32)};
                    } else {
                        if (x.np >= 1) { qpar[0] = ROOT; qkey[0] = x.pk0; qmeta[0] = 1u | slow_flags(x.pf0); }
                        if (x.np >= 2) { qpar[1] = ROOT; qkey[1] = x.pk1; qmeta[1] = 1u | slow_flags(x.pf1); }
                    }
                    if (x.ne >= 1) { ofid[0] = x.ef0; okey[0] = x.ek0; }
                }
                qn = __shfl(x.np, 0, 64);
                on = __shfl(x.ne, 0, 64);
                if (!in_lds) __threadfence_block();
                __syncthreads();
            }
            while (qn > 0) {
                const uint32_t k = min(qn, 64u);
                const bool has = lane < k;
                const uint32_t idx = qn - k + lane;
                uint32_t parent = 0, meta = 0;
                unsigned long long key = 0;
                if (has) {
                    if (in_lds) {
                        const uint4 e = sq[CK_(idx, SLOW_SQ, 27)];
                        parent = e.x; meta = e.y; key = ((unsigned long long)e.w << 32) | e.z;
                    } else {
                        const uint32_t ci = CK_(idx, a.s_qcap, 27);
                        parent = qpar[ci]; meta = qmeta[ci]; key = qkey[ci];
                    }
                }
                if (!in_lds) __threadfence_block();
                __syncthreads();   // every entry popped before the pushes reuse their places
                qn -= k;
                const uint32_t lc = meta & SM_LVL;
                uint32_t pw = W_PLUS;
                if (has && !(meta & SM_PLUS)) pw = w[CK_(lc - 1, d, 28)] & WID_MASK;
                Node s;
                const bool found = has && probe<CK, BIG>(a, parent, pw, s);
                Expand x; x.ne = 0; x.np = 0;
                if (found) {
                    if (!(meta & SM_DSTART)) tV += 1;
                    if (s.flags & NF_HASH) tH += 1;
                    const uint32_t fl2 = (meta & SM_SKIPE) ? M_SKIPE : 0u;
                    expand(s, lc, d, fl2, key, lc < d ? w[CK_(lc, d, 29)] : 0u, w[CK_(lc - 1, d, 28)], x);
                }
                const uint64_t b0 = __ballot(x.np >= 1), b1 = __ballot(x.np >= 2);
                const uint64_t e0 = __ballot(x.ne >= 1), e1 = __ballot(x.ne >= 2);
                const uint32_t ptot = __popcll(b0) + __popcll(b1);
                const uint32_t etot = __popcll(e0) + __popcll(e1);
                if (in_lds && qn + ptot > lcap) { spill = true; break; }
                if (qn + ptot > a.s_qcap || on + etot > a.s_ocap) { err = true; break; }
                const uint32_t pre = prefix_count(b0) + prefix_count(b1);
                const uint32_t m0 = (lc + 1) | slow_flags(x.pf0), m1 = (lc + 1) | slow_flags(x.pf1);
                if (in_lds) {
                    if (x.np >= 1) sq[qn + pre] = uint4{s.child, m0, (uint32_t)x.pk0, (uint32_t)(x.pk0 >> 32)};
                    if (x.np >= 2) sq[qn + pre + 1] = uint4{s.child, m1, (uint32_t)x.pk1, (uint32_t)(x.pk1 >> 32)};
                } else {
                    if (x.np >= 1) { const uint32_t p = qn + pre; qpar[p] = s.child; qkey[p] = x.pk0; qmeta[p] = m0; }
                    if (x.np >= 2) { const uint32_t p = qn + pre + 1; qpar[p] = s.child; qkey[p] = x.pk1; qmeta[p] = m1; }
                }
                qn += ptot;
                const uint32_t epre = prefix_count(e0) + prefix_count(e1);
                if (x.ne >= 1) { ofid[on + epre] = x.ef0; okey[on + epre] = x.ek0; }
                if (x.ne >= 2) { ofid[on + epre + 1] = x.ef1; okey[on + epre + 1] = x.ek1; }
                on += etot;
                if (!in_lds) __threadfence_block();
                __syncthreads();
            }
            if (spill) {
                if (lane == 0) atomicAdd(&a.ctrl[CTRL_SLOW_RESTARTS], 1u);
                in_lds = false;
                __syncthreads();
                continue;
            }
            sV += tV; sH += tH; sW += tW;
            break;
        }
        if (err) {
            if (lane == 0) atomicOr(&a.ctrl[CTRL_ERR], ERR_SLOW_SCRATCH);
            __syncthreads();
            continue;
        }
        __threadfence_block();   // this wave's emissions, read back below
        __syncthreads();
        // sort the row (path code | filter id, or filter bytes for deep /
        // irregular topics), in LDS when it fits
        uint32_t np2 = 1;
        while (np2 < on) np2 <<= 1;
        bool sorted_in_lds = false;
        uint32_t two_runs = 0;   // > 0: sorted as two runs, the second this long (merge_runs_out)
        if (on > 1) {
            if (!by_bytes && np2 > SORT_LDS && on <= 2 * SORT_LDS) {
                // run A: the first SORT_LDS entries, sorted in LDS, back to okey[]
                for (uint32_t i = lane; i < SORT_LDS; i += 64) sk[i] = okey[i] | ofid[i];
                __syncthreads();
                bitonic_lds64(sk, SORT_LDS);
                for (uint32_t i = lane; i < SORT_LDS; i += 64) okey[i] = sk[i];
                __threadfence_block();
                __syncthreads();
                // run B: the rest, sorted in LDS where it stays
                const uint32_t nb = on - SORT_LDS;
                uint32_t nb2 = 1;
                while (nb2 < nb) nb2 <<= 1;
                for (uint32_t i = lane; i < nb2; i += 64)
                    sk[i] = i < nb ? (okey[SORT_LDS + i] | ofid[SORT_LDS + i]) : ~0ull;
                __syncthreads();
                if (nb2 > 1) bitonic_lds64(sk, nb2);
                two_runs = nb;
            } else if (!by_bytes && np2 <= SORT_LDS) {
                // (path codes use bits 31..63, filter ids < 2^30: one u64
                // orders by code, then id)
                for (uint32_t i = lane; i < np2; i += 64) sk[i] = i < on ? (okey[i] | ofid[i]) : ~0ull;
                __syncthreads();
                bitonic_lds64(sk, np2);
                sorted_in_lds = true;
            } else if (by_bytes && np2 <= 2 * SORT_LDS) {
                for (uint32_t i = lane; i < np2; i += 64) sfi[i] = i < on ? ofid[i] : NONE;
                __syncthreads();
                bitonic_lds_bytes<CK>(a, sfi, np2);
                sorted_in_lds = true;
            } else if (np2 <= a.s_ocap) {
                for (uint32_t i = on + lane; i < np2; i += 64) { okey[i] = ~0ull; ofid[i] = NONE; }
                __threadfence_block();
                __syncthreads();
                bitonic<CK>(a, okey, ofid, np2, by_bytes);
            } else {
                if (lane == 0) atomicOr(&a.ctrl[CTRL_ERR], ERR_SLOW_SCRATCH);
                __syncthreads();
                continue;
            }
            __threadfence_block();
            __syncthreads();
        }
        unsigned long long base = 0;
        const uint32_t g = (blockIdx.x % TICKET_GROUPS) & a.sgmask;
        if (lane == 0 && on) base = atomicAdd(xg_top(a.xg, g), (unsigned long long)on);
        base = __shfl(base, 0, 64);
        const bool fits = base + on <= a.rcap;
        base += (uint64_t)g * a.rcap;
        if (fits && two_runs) {
            (void)CK_(base + on - 1, a.sfids_cap, 30);
            merge_runs_out(okey, sk, two_runs, a.sfids + base);
        } else if (fits) {
            for (uint32_t i = lane; i < on; i += 64) {
                const uint32_t f = !sorted_in_lds ? ofid[i] : by_bytes ? sfi[i] : (uint32_t)(sk[i] & ~KEY_MASK);
                a.sfids[CK_(base + i, a.sfids_cap, 30)] = f;
            }
        } else if (lane == 0) {
            atomicOr(&a.ctrl[CTRL_ERR], ERR_STAGING);
        }
        if (lane == 0) { a.count[t] = on; a.src[t] = base; }
        sM += (lane == 0) ? on : 0;
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) {
        sV += __shfl_xor(sV, o, 64); sH += __shfl_xor(sH, o, 64);
        sW += __shfl_xor(sW, o, 64); sM += __shfl_xor(sM, o, 64);
    }
    if (lane == 0 && sS) {
        atomicAdd(&a.stats[ST_VISITS], sV); atomicAdd(&a.stats[ST_HASH], sH);
        atomicAdd(&a.stats[ST_WORDS], sW); atomicAdd(&a.stats[ST_MATCHES], sM);
        atomicAdd(&a.stats[ST_SLOW], sS);
    }
}

// ------------------------------------------------------------ CSR build

constexpr uint32_t SCAN_BLOCK = 1024;
constexpr uint32_t SCAN_PER_THREAD = 4;
constexpr uint32_t SCAN_TILE = SCAN_BLOCK * SCAN_PER_THREAD;

uint32_t scan_block_count(uint32_t n) { return (n + SCAN_TILE - 1) / SCAN_TILE; }

__device__ uint32_t block_excl_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(incl, o, 64);
        if (lane >= (uint32_t)o) incl += u;
    }
    if (lane == 63) sh[wid] = incl;
    __syncthreads();
    if (wid == 0) {
        const uint32_t nw = blockDim.x >> 6;
        const uint32_t s = lane < nw ? sh[lane] : 0;
        uint32_t si = s;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(si, o, 64);
            if (lane >= (uint32_t)o) si += u;
        }
        if (lane < nw) sh[lane] = si - s;
        if (lane == nw - 1) sh[32] = si;
    }
    __syncthreads();
    total = sh[32];
    const uint32_t r = sh[wid] + incl - v;
    __syncthreads();
    return r;
}

// Pass 1: per-block exclusive scan of count[] (slow/overflow rows included).
// A single-block scan (n <= SCAN_TILE: small batches) is final here: block
// offset 0, total -> row_off[n] and *d_total, and pass 2 is not launched.
__global__ __launch_bounds__(SCAN_BLOCK) void tm_scan_local(ScanArgs a, uint32_t* d_total) {
    __shared__ uint32_t sh[33];
    const uint32_t base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_PER_THREAD;
    uint32_t v[SCAN_PER_THREAD];
    uint32_t s = 0;
#pragma unroll
    for (uint32_t i = 0; i < SCAN_PER_THREAD; ++i) {
        v[i] = (base + i < a.n) ? a.count[base + i] : 0u;
        s += v[i];
    }
    uint32_t tot;
    uint32_t ex = block_excl_scan(s, sh, tot);
#pragma unroll
    for (uint32_t i = 0; i < SCAN_PER_THREAD; ++i) {
        if (base + i < a.n) a.row_off[base + i] = ex;
        ex += v[i];
    }
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            a.block_sums[0] = 0;
            a.row_off[a.n] = tot;
            if (d_total) *d_total = tot;
        } else {
            a.block_sums[blockIdx.x] = tot;
        }
    }
}

// Pass 2: exclusive scan of the block sums (single block), total -> row_off[n].
__global__ __launch_bounds__(SCAN_BLOCK) void tm_scan_sums(ScanArgs a, uint32_t nblocks, uint32_t* d_total) {
    __shared__ uint32_t sh[33];
    uint64_t carry = 0;   // u64: a total past u32 is flagged, never wrapped silently
    for (uint32_t b0 = 0; b0 < nblocks; b0 += SCAN_BLOCK) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < nblocks ? a.block_sums[i] : 0u;
        uint32_t tot;
        const uint32_t ex = block_excl_scan(v, sh, tot);
        if (i < nblocks) a.block_sums[i] = (uint32_t)(carry + ex);
        carry += tot;
    }
    if (threadIdx.x == 0) {
        a.row_off[a.n] = (uint32_t)carry;
        if (d_total) *d_total = (uint32_t)carry;
        if (carry > MAX_RESULT && a.ctrl) atomicOr(&a.ctrl[CTRL_ERR], ERR_CSR_RANGE);
    }
}

// Pass 3: one wavefront per tile of 64 topics.  Finishes the CSR offsets and
// copies the tile's sorted rows from the staging region.  A tile whose rows were
// staged as one run (no slow-path topic in it) is one contiguous copy, FIN_U
// coalesced dword loads in flight per lane; otherwise each topic is copied on
// its own.  The next tile's (count, src, offset) are loaded before this tile's
// copy, so a tile costs the copy's round trips, not one more for its header.
template <bool CK>
__global__ __launch_bounds__(64) void tm_finalize(ScanArgs a) {
    const uint32_t lane = threadIdx.x;
    const uint32_t ntiles = (a.n + TILE - 1) / TILE;
    uint32_t nc = 0, noff = 0, nbs = 0;
    uint64_t ns = 0;
    auto meta = [&](uint32_t tile) {
        const uint32_t t = tile * TILE + lane;
        if (tile < ntiles && t < a.n) {
            nc = a.count[t];
            ns = a.src[t];
            noff = a.row_off[t];
            nbs = a.block_sums[t / SCAN_TILE];
        }
    };
    meta(blockIdx.x);
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t t = tile * TILE + lane;
        const bool valid = t < a.n;
        uint32_t c = 0, off = 0;
        uint64_t s = 0;
        if (valid) {
            c = nc;
            s = ns;
            off = noff + nbs;
            a.row_off[t] = off;      // finish the CSR offsets (scan pass 1 was block-local)
        }
        meta(tile + gridDim.x);
        const bool any = c > 0;
        const uint64_t m = __ballot(any);
        if (!m) continue;
        const uint64_t delta = s - (uint64_t)off;
        const uint32_t first = (uint32_t)__builtin_ctzll(m);
        const uint32_t last = 63u - (uint32_t)__builtin_clzll(m);
        const uint64_t d0 = __shfl(delta, first, 64);
        if (__ballot(any && delta != d0) == 0) {
            const uint32_t lo = __shfl(off, first, 64);
            const uint32_t hi = __shfl(off + c, last, 64);
            const uint64_t sb = (uint64_t)lo + d0;
            if ((uint64_t)hi > a.ids_cap || sb + (hi - lo) > a.sfids_cap) continue;   // rerun path
            // FIN_U loads per lane in flight before the stores: a tile's run
            // (~1,500 ids at C2) is one or two memory round trips
            constexpr uint32_t FIN_U = 16;
            for (uint32_t i = lo + lane; i < hi; i += 64 * FIN_U) {
                uint32_t v[FIN_U];
#pragma unroll
                for (uint32_t u = 0; u < FIN_U; ++u) {
                    const uint32_t iu = i + 64 * u;
                    v[u] = iu < hi ? a.sfids[CK_(sb + (iu - lo), a.sfids_cap, 30)] : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < FIN_U; ++u) {
                    const uint32_t iu = i + 64 * u;
                    if (iu < hi) a.ids[CK_(iu, a.ids_cap, 34)] = v[u];
                }
            }
        } else if (any && s + c <= a.sfids_cap && (uint64_t)off + c <= a.ids_cap) {
            for (uint32_t i = 0; i < c; ++i) a.ids[CK_((uint64_t)off + i, a.ids_cap, 38)] = a.sfids[CK_(s + i, a.sfids_cap, 39)];
        }
    }
}

// ------------------------------------------------ routes (emqx_broker:aggre/1)

// Routes per topic = sum over its matched filters of their dest counts
// (lookup_routes/1 for every To in [Topic | Matched], src/emqx_router.erl:132;
// the topic itself is in the trie, so Matched already holds an exact route).
// Routes of a batch = for every match entry, the dests of its filter, in
// match order (emqx_router:match_routes/1 + aggre/1 per publish,
// src/emqx_router.erl:127-133, src/emqx_broker.erl:250-261): the route CSR is
// an exclusive scan of per-ENTRY dest counts, and a topic's first route is its
// first entry's offset.  One thread per entry in each kernel.
__global__ __launch_bounds__(256) void tm_route_count(RouteArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const uint32_t f = a.ids[i];
    a.ecount[i] = f < a.nnodes ? a.roff[f + 1] - a.roff[f] : 0u;
}
__device__ __forceinline__ uint32_t route_eoff(const RouteArgs& a, uint32_t j) {
    return j < a.m ? a.eoff[j] + a.bsums[j / SCAN_TILE] : *a.total;
}
__global__ __launch_bounds__(256) void tm_route_rows(RouteArgs a) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t <= a.n) a.r_rowoff[t] = route_eoff(a, a.row_off[t]);
}
__global__ __launch_bounds__(256) void tm_route_fill(RouteArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const uint32_t f = a.ids[i];
    if (f >= a.nnodes) return;
    uint64_t o = route_eoff(a, i);
    for (uint32_t k = a.roff[f], ke = a.roff[f + 1]; k < ke && o < a.cap; ++k, ++o) {
        a.out_fid[o] = f;
        a.out_dest[o] = a.rdest[k];
    }
}

// ----------------------- shared subscriptions (emqx_shared_sub:dispatch/3)
//
// do_route({To, Group}, Delivery) (src/emqx_broker.erl:245-248) for every
// matched filter To of every publish: one delivery per group run on the
// filter, the member picked by pick_subscriber/5 (src/emqx_shared_sub.erl:
// 260-275).  Entry-parallel like the routes: count = groups on the entry's
// filter (a 1-B gather, most entries stop there), the u32 scan, then one
// thread per entry picks for each of its runs.  Only an entry with groups
// looks for its publish (a binary search of the match CSR's row offsets).

__global__ __launch_bounds__(256) void tm_shared_count(SharedArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    uint32_t c = 0;
    if (i < a.m) {
        const uint32_t f = a.ids[i];
        if (f < a.nnodes) {
            c = a.gcnt[f];
            if (c == 255) c = a.goff[f + 1] - a.goff[f];
        }
        a.ecount[i] = c;
    }
    unsigned long long s = c;
    for (int o = 32; o; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(a.total64, s);
}
__device__ __forceinline__ uint32_t shared_eoff(const SharedArgs& a, uint32_t j) {
    return j < a.m ? a.eoff[j] + a.bsums[j / SCAN_TILE] : *a.total;
}
__global__ __launch_bounds__(256) void tm_shared_rows(SharedArgs a) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t <= a.n) a.g_rowoff[t] = shared_eoff(a, a.row_off[t]);
}
__device__ __forceinline__ unsigned long long shared_mix(unsigned long long z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__global__ __launch_bounds__(256) void tm_shared_pick(SharedArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.m) return;
    const uint32_t f = a.ids[i];
    if (f >= a.nnodes || a.gcnt[f] == 0) return;
    // the publish of entry i: the last row p with row_off[p] <= i (rows before it may be empty)
    uint32_t lo = 0, hi = a.n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.row_off[mid] <= i) lo = mid; else hi = mid;
    }
    const uint32_t p = lo;
    uint64_t o = shared_eoff(a, i);
    const uint32_t ke = min(a.goff[f + 1], a.nruns);
    for (uint32_t k = a.goff[f]; k < ke && o < a.cap; ++k, ++o) {
        const uint4 run = a.runs[k];   // group, first member, count, slot
        const uint32_t cnt = run.z;
        uint32_t nth = 0;
        if (cnt > 1) {   // [Sub] -> Sub: no state, no key (:260)
            if (a.strategy == SH_HASH) {
                nth = a.keys[p] % cnt;
            } else if (a.strategy == SH_ROUND_ROBIN) {
                if (run.w < a.nslots) nth = (uint32_t)(atomicAdd(&a.slots[run.w].cur, 1ull) % cnt);
            } else {
                constexpr unsigned long long G = 0x9E3779B97F4A7C15ull;
                unsigned long long z = shared_mix(a.seed + G * ((unsigned long long)p + 1));
                z = shared_mix((z ^ ((unsigned long long)f << 32 | run.x)) + G);
                nth = (uint32_t)(z >> 32) % cnt;
            }
        }
        const uint64_t mi = (uint64_t)run.y + nth;
        a.out_fid[o] = f;
        a.out_grp[o] = run.x;
        a.out_sub[o] = (cnt && mi < a.nmem) ? a.mem[mi] : NONE;
        if (a.out_ent) a.out_ent[o] = i;
    }
}
// A new build of the tables reached the replica: upd[s] = {member count, owner
// epoch} of run slot s.  A slot whose owner changed starts over (the first pick
// ever is member 1).  A slot that was picked from since its last fold stores
// the reference's remainder N = last pick index as cur = N + 1
// (src/emqx_shared_sub.erl:270-274), so the next pick under the new count is
// (N + 1) rem NewCount; one that was not picked from keeps its N.
__global__ __launch_bounds__(256) void tm_shared_fold(SharedSlot* slots, const uint2* upd, uint32_t nslots) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nslots) return;
    SharedSlot v = slots[s];
    const uint2 u = upd[s];
    if (v.epoch != u.y) {
        v.cur = v.base = 0;
        v.epoch = u.y;
    } else if (v.cur != v.base && v.cnt) {
        v.cur = v.base = (v.cur - 1) % v.cnt + 1;
    }
    v.cnt = u.x;
    slots[s] = v;
}

// ------------------------------------------ fan-out (emqx_broker:dispatch/2)
//
// dispatch(To, Delivery) folds over subscribers(To) for every local route of the
// publish (src/emqx_broker.erl:243-244, 284-309).  The match CSR already lists
// the publish's filters in order, so the deliveries of a batch are the
// concatenation, over match entries j, of the subscriber run of filter ids[j]:
//   scan  moff[j] = sum of the run lengths before entry j (u64: a hot filter can
//         carry millions of subscribers), drow[i] = moff[row_off[i]];
//   fill  one thread per DELIVERY, not per publish or filter: a workgroup owns
//         4096 consecutive outputs, finds the entries covering them by binary
//         search of moff, and copies subscriber ids with coalesced loads and
//         stores -- balanced whatever the fan-out skew (1 vs 10^6 subscribers).

constexpr uint32_t FAN_BLOCK = 256;
constexpr uint32_t FAN_PER = 16;                           // entries per scan thread
constexpr uint32_t FAN_SCAN_TILE = FAN_BLOCK * FAN_PER;
#ifndef TM_FAN_FILL_PER
#define TM_FAN_FILL_PER 8
#endif
constexpr uint32_t FAN_FILL_PER = TM_FAN_FILL_PER;         // deliveries per fill thread (8 or 16)
static_assert(FAN_FILL_PER % 8 == 0 && FAN_FILL_PER >= 8, "the fill's max-scan reads its marks as uint4 words (8 per thread)");
constexpr uint32_t FAN_FILL_TILE = FAN_BLOCK * FAN_FILL_PER;
constexpr uint32_t FAN_LDS_ENTRIES = FAN_FILL_TILE * 3 / 4;  // match entries a fill tile can stage

// first delivery of match entry j: the block's offset plus the block-relative
// u32 (u64 only in scan blocks with 2^32 deliveries or more)
__device__ inline uint64_t fan_moff(const FanArgs& a, uint64_t j) {
    // the u32 offset, the block flag and the block sum are loaded together
    // (moff32 spans every entry, so the speculative read is in bounds); only a
    // block past 2^32 deliveries reads the u64 offset after the flag
    const uint64_t b = j / FAN_SCAN_TILE;
    const uint32_t m32 = a.moff32[j];
    const bool big = a.bbig[b] != 0;
    const uint64_t bs = a.bsums[b];
    return (big ? a.moff[j] : (uint64_t)m32) + bs;
}

// Rows mode: region of virtual entry j (vb[0] = 0, vb ascending)
__device__ __forceinline__ uint32_t fan_region(const FanArgs& a, uint64_t j) {
    uint32_t g = 0;
#pragma unroll
    for (uint32_t k = 1; k < TICKET_GROUPS; ++k) g += (k < a.nreg && j >= a.vb[k]) ? 1u : 0u;
    return g;
}

// filter id of entry j (rows mode: the staging entry behind it; padding ->
// nnodes, i.e. no deliveries)
__device__ __forceinline__ uint32_t fan_fid(const FanArgs& a, uint64_t j) {
    if (!a.nreg) return a.ids[j];
    const uint32_t g = fan_region(a, j);
    const uint64_t o = j - a.vb[g];
    return o < a.rtop[g] ? a.ids[g * a.rcap + o] : a.nnodes;
}

// Exclusive scan of one u64 per thread over a 256-thread block (4 waves).
__device__ inline uint64_t fan_block_scan(uint64_t v, uint64_t* lds, uint64_t& total) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    uint64_t base = 0;
    for (uint32_t k = 0; k < w; ++k) base += lds[k];
    total = lds[0] + lds[1] + lds[2] + lds[3];
    __syncthreads();
    return base + x - v;
}

// A block scans FAN_SCAN_TILE entries as FAN_PER striped chunks of FAN_BLOCK
// (coalesced ids loads and moff stores); all chunks' run lengths are gathered
// before the first scan so the soff loads overlap.  The block's total decides
// the width of its offsets: u32 (half the bytes every reader moves) unless the
// block delivers 2^32 or more (a hot filter with millions of subscribers).
__global__ __launch_bounds__(FAN_BLOCK) void tm_fan_scan_local(FanArgs a) {
    __shared__ uint64_t lds[4];
    // thread t owns FAN_PER consecutive entries: a serial prefix in registers
    // and ONE block scan of the per-thread sums (striped chunks needed one
    // block scan per chunk); ids and offsets move as 16-B vectors
    const uint64_t j0 = (uint64_t)blockIdx.x * FAN_SCAN_TILE + (uint64_t)threadIdx.x * FAN_PER;
    uint32_t f[FAN_PER];
    // rows mode: the 16 entries lie in one region (its virtual base and the
    // region stride are multiples of 16), so they are one aligned chunk of
    // staging; entries past the region's top are padding
    const uint32_t* src = a.ids + j0;
    uint64_t valid = a.n_matches > j0 ? a.n_matches - j0 : 0;
    if (a.nreg && valid) {
        const uint32_t g = fan_region(a, j0);
        const uint64_t o = j0 - a.vb[g];
        src = a.ids + g * a.rcap + o;
        valid = a.rtop[g] > o ? min<uint64_t>(valid, a.rtop[g] - o) : 0;
    }
    if (j0 + FAN_PER <= a.n_matches) {
        const uint4* q = reinterpret_cast<const uint4*>(src);   // 64-B aligned
#pragma unroll
        for (uint32_t k = 0; k < FAN_PER / 4; ++k) {
            const uint4 v = q[k];
            f[4 * k] = v.x; f[4 * k + 1] = v.y; f[4 * k + 2] = v.z; f[4 * k + 3] = v.w;
        }
#pragma unroll
        for (uint32_t k = 0; k < FAN_PER; ++k)
            if (k >= valid) f[k] = a.nnodes;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < FAN_PER; ++k) f[k] = k < valid ? src[k] : a.nnodes;
    }
    uint64_t c[FAN_PER], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < FAN_PER; ++k) {
        c[k] = 0;
        if (f[k] < a.nnodes) {
            const uint32_t s1 = a.scnt[f[k]];   // 1 B per node: the gather's footprint stays L2-sized
            c[k] = s1 < 255 ? s1 : a.soff[f[k] + 1] - a.soff[f[k]];
        }
        mine += c[k];
    }
    uint64_t total;
    uint64_t run = fan_block_scan(mine, lds, total);
    const bool big = total > a.big_limit;
    if (!big && j0 + FAN_PER <= a.n_matches + 1) {
        uint4* q = reinterpret_cast<uint4*>(a.moff32 + j0);
#pragma unroll
        for (uint32_t k = 0; k < FAN_PER / 4; ++k) {
            uint4 v;
            v.x = (uint32_t)run; run += c[4 * k];
            v.y = (uint32_t)run; run += c[4 * k + 1];
            v.z = (uint32_t)run; run += c[4 * k + 2];
            v.w = (uint32_t)run; run += c[4 * k + 3];
            q[k] = v;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < FAN_PER; ++k) {
            const uint64_t j = j0 + k;
            if (j <= a.n_matches) {
                if (big) a.moff[j] = run;
                else a.moff32[j] = (uint32_t)run;
            }
            run += c[k];
        }
    }
    if (threadIdx.x == 0) {
        a.bsums[blockIdx.x] = total;
        a.bbig[blockIdx.x] = big ? 1 : 0;
    }
}

__global__ __launch_bounds__(FAN_BLOCK) void tm_fan_scan_sums(FanArgs a, uint32_t nb) {
    // each thread owns a contiguous chunk of the block sums: a serial sum, ONE
    // block scan of the chunk sums, then a serial exclusive pass (one block
    // scan per 256 sums made this a long chain of barriers at 60k blocks)
    __shared__ uint64_t lds[4];
    const uint32_t per = (nb + FAN_BLOCK - 1) / FAN_BLOCK;
    const uint32_t lo = min(nb, threadIdx.x * per), hi = min(nb, lo + per);
    // 8 loads of a chunk in flight at a time (a dependent chain of 230 loads
    // per thread was the cost); the chunk is kept in registers for pass 2 when
    // it fits
    constexpr uint32_t U = 8;
    uint64_t mine = 0;
    for (uint32_t i0 = lo; i0 < hi; i0 += U) {
        uint64_t v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = i0 + u < hi ? a.bsums[i0 + u] : 0ull;
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) mine += v[u];
    }
    uint64_t total;
    uint64_t run = fan_block_scan(mine, lds, total);
    for (uint32_t i0 = lo; i0 < hi; i0 += U) {
        uint64_t v[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) v[u] = i0 + u < hi ? a.bsums[i0 + u] : 0ull;
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            if (i0 + u < hi) a.bsums[i0 + u] = run;
            run += v[u];
        }
    }
    if (threadIdx.x == 0) *a.d_total = total;
}

// After scan_local + scan_sums, moff32[j] (or moff[j] in a big block) is
// relative to its scan block and bsums[b] is the block's exclusive offset:
// rows, tiles and fill read the sum (bsums is small and cache-resident).
// tm_fan_scan_add writes the global u64 offsets into moff -- only when the
// caller asks for the match offsets, and only after the fill.
__global__ __launch_bounds__(FAN_BLOCK) void tm_fan_scan_add(FanArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * FAN_BLOCK + threadIdx.x;
    if (j <= a.n_matches) a.moff[j] = fan_moff(a, j);   // in place for big blocks: read, then write
}

__global__ __launch_bounds__(FAN_BLOCK) void tm_fan_rows(FanArgs a) {
    const uint32_t i = blockIdx.x * FAN_BLOCK + threadIdx.x;
    if (i <= a.n) a.drow[i] = fan_moff(a, a.row_off[i]);
}

// rows mode: the deliveries of publish i's row, read where the walk left it
// (count, first staging entry): first delivery and count
__global__ __launch_bounds__(FAN_BLOCK) void tm_fan_rows_stg(FanArgs a) {
    const uint32_t i = blockIdx.x * FAN_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t c = a.rcount[i];
    uint64_t d0 = 0, dn = 0;
    if (c) {
        const uint64_t s = a.rsrc[i];
        const uint32_t g = a.nreg > 1 ? (uint32_t)(s / a.rcap) : 0u;
        const uint64_t v = a.vb[g] + (s - g * a.rcap);
        d0 = fan_moff(a, v);
        dn = fan_moff(a, v + c) - d0;
    }
    a.drow[i] = d0;
    a.dcount[i] = (uint32_t)dn;
}

// first j in [lo, hi) with moff[j] > p (hi if none)
__device__ inline uint64_t fan_upper(const FanArgs& a, uint64_t lo, uint64_t hi, uint64_t p) {
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (fan_moff(a, m) > p) hi = m;
        else lo = m + 1;
    }
    return lo;
}

// tile_j[k] = match entry of delivery k * FAN_FILL_TILE (k < ntiles), and
// tile_j[ntiles] = entry of the last delivery: one search per tile, all tiles
// at once, instead of a dependent search chain at the head of every fill block.
__global__ __launch_bounds__(FAN_BLOCK) void tm_fan_tiles(FanArgs a, uint64_t ntiles) {
    const uint64_t k = (uint64_t)blockIdx.x * FAN_BLOCK + threadIdx.x;
    if (k > ntiles) return;
    const uint64_t p = k < ntiles ? k * FAN_FILL_TILE : a.total - 1;
    a.tile_j[k] = fan_upper(a, 0, a.n_matches + 1, p) - 1;
}

// One workgroup per 4096 consecutive deliveries.  The entries covering the
// tile (jlo..jhi) are staged in LDS: each non-empty run marks its first
// delivery in the tile with its entry index and keeps soff[f] - moff[j]; an
// inclusive max-scan over the marks gives every delivery its entry, and the
// copy is then one LDS read + one subscriber load + one coalesced store per
// delivery.  A tile covering more than FAN_LDS_ENTRIES entries (long stretches
// of filters without local subscribers) searches moff per delivery instead.
// WIDE: the batch delivers more than big_limit (some scan block may hold u64
// offsets); otherwise only the 32-bit staging path is compiled in
// WJ (tm_batch_inboxes): the entry of every delivery goes to out_j as well --
// the max-scan has it already, so it is one more coalesced store
template <bool WIDE, bool WJ = false>
__global__ __launch_bounds__(FAN_BLOCK) void tm_fan_fill(FanArgs a) {
    __shared__ int64_t base[FAN_LDS_ENTRIES];
    __shared__ __attribute__((aligned(16))) uint16_t own[FAN_FILL_TILE];
    __shared__ uint32_t wmax[FAN_BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t start = (uint64_t)blockIdx.x * FAN_FILL_TILE;
    const uint64_t end = min(start + FAN_FILL_TILE, a.total);
    const uint32_t len = (uint32_t)(end - start);
    const uint64_t jlo = a.tile_j[blockIdx.x];
    const uint64_t jhi = a.tile_j[blockIdx.x + 1];
    const uint64_t ne = jhi - jlo + 1;
    if (ne > FAN_LDS_ENTRIES) {
        // moff[j] <= p < moff[j + 1] for the entry of delivery p; p only grows
        // per thread, so each search starts at the previous entry
        uint64_t j = jlo;
        for (uint64_t p = start + t; p < end; p += FAN_BLOCK) {
            j = fan_upper(a, j, jhi + 1, p) - 1;
            a.out[p] = a.subs[a.soff[fan_fid(a, j)] + (p - fan_moff(a, j))];
            if constexpr (WJ) a.out_j[p] = (uint32_t)j;
        }
        return;
    }
    uint4* own4 = reinterpret_cast<uint4*>(own);
    for (uint32_t i = t; i < FAN_FILL_TILE / 8; i += FAN_BLOCK) own4[i] = make_uint4(0, 0, 0, 0);
    // The entries [jlo, jhi + 1] lie in at most two scan blocks (ne + 1 <=
    // FAN_LDS_ENTRIES + 1 < FAN_SCAN_TILE): their "big" flags and offsets are
    // read once, so an entry's delivery offset is one load, not a flag load
    // and then the offset load.
    const uint64_t sb0 = jlo / FAN_SCAN_TILE;
    const uint64_t nsb = a.n_matches / FAN_SCAN_TILE + 1;   // scan blocks over n_matches + 1 entries
    const bool big0 = a.bbig[sb0], big1 = sb0 + 1 < nsb ? a.bbig[sb0 + 1] != 0 : false;
    const uint64_t bs0 = a.bsums[sb0], bs1 = sb0 + 1 < nsb ? a.bsums[sb0 + 1] : 0;
    auto moff_at = [&](uint64_t j) -> uint64_t {
        const bool hi = j / FAN_SCAN_TILE != sb0;
        return ((hi ? big1 : big0) ? a.moff[j] : (uint64_t)a.moff32[j]) + (hi ? bs1 : bs0);
    };
    __syncthreads();
    // rows mode: a tile's entries usually lie in one staging region, whose
    // entries are then one offset away (padding entries have no deliveries,
    // so whatever they read is never used); a tile across regions maps each
    const bool one_reg = !a.nreg || fan_region(a, jlo) == fan_region(a, jhi + 1);
    const uint32_t* fids = a.ids;
    if (a.nreg && one_reg) {
        const uint32_t g = fan_region(a, jlo);
        fids = a.ids + g * a.rcap - a.vb[g];
    }
    // staging, FAN_STG entries per thread with every load of a step in flight
    // (the offsets and filter ids, then the dependent sone / soff gathers)
#ifndef TM_FAN_STG
#define TM_FAN_STG 8
#endif
    constexpr uint32_t FAN_STG = TM_FAN_STG;
    if (!WIDE || (!big0 && !big1)) {
        // both scan blocks of the tile's entries hold u32 offsets (the common
        // case): the loads stay 32-bit until the gathers are issued
        for (uint32_t e0 = t; e0 < (uint32_t)ne; e0 += FAN_BLOCK * FAN_STG) {
            uint32_t r0[FAN_STG], r1[FAN_STG], f[FAN_STG];
#pragma unroll
            for (uint32_t u = 0; u < FAN_STG; ++u) {
                const uint32_t e = e0 + u * FAN_BLOCK;
                r0[u] = 0; r1[u] = 0; f[u] = 0;
                if (e < (uint32_t)ne) {
                    const uint64_t j = jlo + e;
                    r0[u] = a.moff32[j];
                    r1[u] = a.moff32[j + 1];
                    f[u] = one_reg ? fids[j] : fan_fid(a, j);
                }
            }
            int64_t v[FAN_STG];
            uint32_t at[FAN_STG];   // my mark's place in own[], NONE: inactive
#pragma unroll
            for (uint32_t u = 0; u < FAN_STG; ++u) {
                const uint64_t j = jlo + e0 + u * FAN_BLOCK;
                const uint64_t m0 = r0[u] + (j / FAN_SCAN_TILE != sb0 ? bs1 : bs0);
                const uint64_t m1 = r1[u] + ((j + 1) / FAN_SCAN_TILE != sb0 ? bs1 : bs0);
                const bool act = e0 + u * FAN_BLOCK < (uint32_t)ne && m1 > m0 && m1 > start && m0 < end;
                v[u] = 0;
                at[u] = act ? (m0 > start ? (uint32_t)(m0 - start) : 0u) : NONE;
                if (act) v[u] = m1 - m0 == 1 ? INT64_MIN + (int64_t)a.sone[f[u]] : (int64_t)a.soff[f[u]] - (int64_t)m0;
            }
#pragma unroll
            for (uint32_t u = 0; u < FAN_STG; ++u) {
                if (at[u] == NONE) continue;
                const uint32_t e = e0 + u * FAN_BLOCK;
                base[e] = v[u];
                own[at[u]] = (uint16_t)(e + 1);
            }
        }
    } else
    for (uint32_t e0 = t; e0 < (uint32_t)ne; e0 += FAN_BLOCK * FAN_STG) {
        uint64_t m0[FAN_STG], m1[FAN_STG];
        uint32_t f[FAN_STG];
        bool act[FAN_STG];
#pragma unroll
        for (uint32_t u = 0; u < FAN_STG; ++u) {
            const uint32_t e = e0 + u * FAN_BLOCK;
            m0[u] = 0; m1[u] = 0; f[u] = 0;
            if (e < (uint32_t)ne) {
                const uint64_t j = jlo + e;
                m0[u] = moff_at(j);
                m1[u] = moff_at(j + 1);
                f[u] = one_reg ? fids[j] : fan_fid(a, j);
            }
        }
        int64_t v[FAN_STG];
#pragma unroll
        for (uint32_t u = 0; u < FAN_STG; ++u) {
            act[u] = m1[u] > m0[u] && m1[u] > start && m0[u] < end;
            v[u] = 0;
            // a one-delivery run keeps its subscriber inline (one 4-B gather,
            // no dependent read of subs[]): INT64_MIN + id marks it
            if (act[u]) v[u] = m1[u] - m0[u] == 1 ? INT64_MIN + (int64_t)a.sone[f[u]]
                                                  : (int64_t)a.soff[f[u]] - (int64_t)m0[u];
        }
#pragma unroll
        for (uint32_t u = 0; u < FAN_STG; ++u) {
            if (!act[u]) continue;
            const uint32_t e = e0 + u * FAN_BLOCK;
            base[e] = v[u];
            own[m0[u] > start ? (uint32_t)(m0[u] - start) : 0u] = (uint16_t)(e + 1);
        }
    }
    __syncthreads();
    // inclusive max-scan of own[] (entry starts only grow along the tile)
    constexpr uint32_t NQ = FAN_FILL_PER / 8;                // uint4 words of marks per thread
    uint32_t v[FAN_FILL_PER];
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) {
        const uint4 u = own4[NQ * t + q];
        const uint32_t wd[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) { v[8 * q + 2 * k] = wd[k] & 0xFFFFu; v[8 * q + 2 * k + 1] = wd[k] >> 16; }
    }
    uint32_t run = 0;
#pragma unroll
    for (uint32_t k = 0; k < FAN_FILL_PER; ++k) { run = max(run, v[k]); v[k] = run; }
    uint32_t x = run;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x = max(x, y);
    }
    if (lane == 63) wmax[w] = x;
    uint32_t pre = __shfl_up(x, 1, 64);
    if (lane == 0) pre = 0;
    __syncthreads();
    for (uint32_t k = 0; k < w; ++k) pre = max(pre, wmax[k]);
#pragma unroll
    for (uint32_t q = 0; q < NQ; ++q) {
        uint32_t o[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            o[k] = max(v[8 * q + 2 * k], pre) | (max(v[8 * q + 2 * k + 1], pre) << 16);
        own4[NQ * t + q] = make_uint4(o[0], o[1], o[2], o[3]);
    }
    __syncthreads();
    // the copy: every delivery's subscriber load of this thread in flight at once
    uint32_t r[FAN_FILL_PER];
#pragma unroll
    for (uint32_t u = 0; u < FAN_FILL_PER; ++u) {
        const uint32_t i = t + u * FAN_BLOCK;
        r[u] = 0;
        if (i < len) {
            const int64_t bs = base[(uint32_t)own[i] - 1u];
            r[u] = bs < INT64_MIN + (1ll << 33) ? (uint32_t)(bs - INT64_MIN)
                                                : a.subs[(uint64_t)(bs + (int64_t)(start + i))];
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < FAN_FILL_PER; ++u) {
        const uint32_t i = t + u * FAN_BLOCK;
        if (i < len) a.out[start + i] = r[u];
    }
    if constexpr (WJ) {
#pragma unroll
        for (uint32_t u = 0; u < FAN_FILL_PER; ++u) {
            const uint32_t i = t + u * FAN_BLOCK;
            if (i < len) a.out_j[start + i] = (uint32_t)(jlo + ((uint32_t)own[i] - 1u));
        }
    }
}

// ------------------------------------- per-subscriber inboxes (tm_batch_inboxes)
//
// SubPid ! {deliver, Topic, Msg} (src/emqx_broker.erl:298-302) for a whole
// batch: the fan-out's deliveries, in publish order, regrouped by subscriber
// with each subscriber's deliveries kept in that order -- a stable sort of
// (subscriber, match entry) pairs.  LSD radix, 8 bits per pass:
//   hist     the pass's digit counts per tile, digit-major
//   scan     (the project's two-level scan) -> the first output slot of (digit, tile)
//   scatter  rank of a pair among the equal digits before it in its tile, from
//            wave ballots (no LDS atomics: a '#' subscriber makes a whole
//            tile one key), staged in LDS by digit, written as runs
// A tile's histogram for pass p counts the pairs the tile holds when pass p
// starts, i.e. as pass p - 1 left them, so tm_inbox_hist runs once per pass on
// that pass's input: one read of the unsorted keys can give every pass's
// GLOBAL histogram but not the per-tile ones a scatter without look-back needs.
// Every kernel terminates on its own inputs.

constexpr uint32_t INBOX_BLOCK = 256;
constexpr uint32_t INBOX_WAVE_PAIRS = INBOX_TILE / (INBOX_BLOCK / 64);   // 1024 consecutive pairs per wave
constexpr uint32_t INBOX_ROUNDS = INBOX_WAVE_PAIRS / 64;                 // of 64 consecutive pairs each
static_assert(MAX_RESULT + 16 <= 0x100000000ull, "a delivery index plus a tile's slack fits u32");

// lanes of the wave whose digit equals mine, among the active ones: 8 ballots,
// the same cost whatever the skew
__device__ __forceinline__ uint64_t inbox_peers(uint32_t d, uint64_t act) {
    uint64_t peers = act;
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
        const bool s = (d >> b) & 1u;
        const uint64_t m = __ballot(s);
        peers &= s ? m : ~m;
    }
    return peers;
}
__device__ __forceinline__ uint32_t inbox_mbcnt(uint64_t m) {   // set bits of m below my lane
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(256) void tm_inbox_pubof(InboxArgs a) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.m) return;
    // the last row p with row_off[p] <= j (rows before it may be empty)
    uint32_t lo = 0, hi = a.n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.row_off[mid] <= j) lo = mid; else hi = mid;
    }
    a.pub_of[j] = lo;
}

// The merged list L' of an armed batch (tm_batch_shared_mode): within a match
// entry the {To, node()} route precedes every {To, Group} route
// (src/emqx_broker.erl:255-261), so entry j holds its ordinary run and then
// its picks.  Delivery-parallel, whatever the skew of the entries: thread t <
// nd moves ordinary delivery t of entry j = fent[t] up by the picks of the
// entries before j; thread nd + s puts pick s (of entry gent[s]) behind the
// ordinary run of its entry, i.e. at moff[j + 1] + s.  Reads are coalesced,
// writes are runs.  Every position of [0, cap) is written once when the
// inputs are consistent; anything else is counted in err and written nowhere.
__global__ __launch_bounds__(256) void tm_inbox_merge(MergeArgs a) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (uint64_t)a.nd + a.ns) return;
    uint32_t S, j, g;
    uint64_t pos;
    if (t < a.nd) {
        S = a.fsub[t];
        j = a.fent[t];
        g = NONE;
        if (j >= a.m) { atomicAdd(a.err, 1u); return; }
        pos = t + a.eoff[j] + a.bsums[j / SCAN_TILE];
    } else {
        const uint32_t s = (uint32_t)(t - a.nd);
        S = a.gsub[s];
        j = a.gent[s];
        g = a.ggrp[s];
        // a group route without a member cannot happen under the engine lock
        if (S == NONE || j >= a.m) { atomicAdd(a.err, 1u); return; }
        pos = a.moff[j + 1] + s;
    }
    if (pos >= a.cap) { atomicAdd(a.err, 1u); return; }
    a.key[pos] = S;
    a.val[pos] = (uint32_t)pos;
    a.rec[pos] = make_uint4(a.pub_of[j], a.ids[j], g, j);
}

// hist[d * ntiles + tile] = pairs of the tile whose digit (key >> shift) & 255 is d
__global__ __launch_bounds__(INBOX_BLOCK) void tm_inbox_hist(InboxArgs a, const uint32_t* keys, uint32_t* hist,
                                                             uint32_t shift) {
    __shared__ uint32_t cnt[INBOX_BLOCK / 64][256];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (uint32_t i = t; i < (INBOX_BLOCK / 64) * 256; i += INBOX_BLOCK) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const uint64_t wbase = (uint64_t)blockIdx.x * INBOX_TILE + (uint64_t)w * INBOX_WAVE_PAIRS;
    uint32_t key[INBOX_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        key[r] = q < a.D ? keys[q] : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const bool on = q < a.D;
        const uint32_t d = (key[r] >> shift) & 255u;
        const uint64_t peers = inbox_peers(d, __ballot(on));
        // the first lane of every digit adds its lanes to the wave's own counter
        if (on && inbox_mbcnt(peers) == 0) cnt[w][d] += (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < INBOX_BLOCK / 64; ++k) s += cnt[k][t];
    hist[(uint64_t)t * a.ntiles + blockIdx.x] = s;   // t = digit (256 threads, 256 digits)
}
static_assert(INBOX_BLOCK == 256, "one thread per digit");

// One pass over one tile: (kin, vin) -> (kout, vout) by digit (key >> shift) & 255.
// off / bs: the pass's scanned table.
__global__ __launch_bounds__(INBOX_BLOCK) void tm_inbox_scatter(InboxArgs a, const uint32_t* kin, const uint32_t* vin,
                                                                uint32_t* kout, uint32_t* vout, const uint32_t* off,
                                                                const uint32_t* bs, uint32_t shift) {
    __shared__ uint32_t sk[INBOX_TILE], sv[INBOX_TILE];
    __shared__ uint32_t cnt[INBOX_BLOCK / 64][256];   // per wave and digit: pairs so far, then the wave's first slot
    __shared__ uint32_t gb[256];                      // per digit: first output slot - first staged slot
    __shared__ uint32_t sh[33];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (uint32_t i = t; i < (INBOX_BLOCK / 64) * 256; i += INBOX_BLOCK) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const uint64_t tbase = (uint64_t)blockIdx.x * INBOX_TILE;
    const uint64_t wbase = tbase + (uint64_t)w * INBOX_WAVE_PAIRS;
    uint32_t key[INBOX_ROUNDS], val[INBOX_ROUNDS], rk[INBOX_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        key[r] = q < a.D ? kin[q] : 0u;
        val[r] = q < a.D ? vin[q] : 0u;
    }
    // rank among the wave's equal digits: earlier rounds (the counter), then lower lanes (mbcnt)
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const bool on = q < a.D;
        const uint32_t d = (key[r] >> shift) & 255u;
        const uint64_t peers = inbox_peers(d, __ballot(on));
        const uint32_t below = inbox_mbcnt(peers);
        const uint32_t c0 = on ? cnt[w][d] : 0u;
        __builtin_amdgcn_wave_barrier();
        if (on && below == 0) cnt[w][d] = c0 + (uint32_t)__popcll(peers);
        __builtin_amdgcn_wave_barrier();
        rk[r] = c0 + below;
    }
    __syncthreads();
    // thread = digit: the digit's first staged slot (scan over the digits), its
    // waves' first slots (earlier waves first), and where its run goes
    {
        uint32_t c[INBOX_BLOCK / 64], tot = 0;
#pragma unroll
        for (uint32_t k = 0; k < INBOX_BLOCK / 64; ++k) { c[k] = cnt[k][t]; tot += c[k]; }
        uint32_t all;
        const uint32_t first = block_excl_scan(tot, sh, all);
        uint32_t run = first;
#pragma unroll
        for (uint32_t k = 0; k < INBOX_BLOCK / 64; ++k) { cnt[k][t] = run; run += c[k]; }
        const uint64_t i = (uint64_t)t * a.ntiles + blockIdx.x;
        gb[t] = off[i] + bs[i / SCAN_TILE] - first;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        if (q < a.D) {
            const uint32_t pos = cnt[w][(key[r] >> shift) & 255u] + rk[r];
            if (pos < INBOX_TILE) { sk[pos] = key[r]; sv[pos] = val[r]; }
        }
    }
    __syncthreads();
    const uint32_t len = (uint32_t)min<uint64_t>(INBOX_TILE, a.D - tbase);
#pragma unroll
    for (uint32_t k = 0; k < INBOX_TILE / INBOX_BLOCK; ++k) {
        const uint32_t s = k * INBOX_BLOCK + t;
        if (s < len) {
            const uint32_t ky = sk[s];
            const uint32_t dst = gb[(ky >> shift) & 255u] + s;
            if (dst < a.D) { kout[dst] = ky; vout[dst] = sv[s]; }
        }
    }
}

// The sorted pairs -> (publish, filter) of every delivery, and the inbox heads
// (the first delivery of every subscriber) of the tile counted.  MERGED (an
// armed batch): the payload is a position of L'; publish, filter and group are
// that position's record.
template <bool MERGED>
__global__ __launch_bounds__(INBOX_BLOCK) void tm_inbox_finish(InboxArgs a, const uint32_t* keys, const uint32_t* vals) {
    __shared__ uint32_t hw[INBOX_BLOCK / 64];
    const uint32_t t = threadIdx.x;
    const uint64_t tbase = (uint64_t)blockIdx.x * INBOX_TILE;
    uint32_t heads = 0;
    uint32_t j[INBOX_TILE / INBOX_BLOCK], ky[INBOX_TILE / INBOX_BLOCK], kp[INBOX_TILE / INBOX_BLOCK];
#pragma unroll
    for (uint32_t k = 0; k < INBOX_TILE / INBOX_BLOCK; ++k) {
        const uint64_t q = tbase + k * INBOX_BLOCK + t;
        j[k] = q < a.D ? vals[q] : a.m;
        ky[k] = q < a.D ? keys[q] : 0u;
        kp[k] = (q < a.D && q) ? keys[q - 1] : ~ky[k];
    }
    uint32_t p[INBOX_TILE / INBOX_BLOCK], f[INBOX_TILE / INBOX_BLOCK];
    if constexpr (MERGED) {
        uint4 rc[INBOX_TILE / INBOX_BLOCK];
#pragma unroll
        for (uint32_t k = 0; k < INBOX_TILE / INBOX_BLOCK; ++k) {
            const uint64_t q = tbase + k * INBOX_BLOCK + t;
            const uint32_t v = j[k];
            rc[k] = (q < a.D && v < a.D) ? a.mrec[v] : make_uint4(NONE, NONE, NONE, NONE);
        }
#pragma unroll
        for (uint32_t k = 0; k < INBOX_TILE / INBOX_BLOCK; ++k) {
            const uint64_t q = tbase + k * INBOX_BLOCK + t;
            p[k] = rc[k].x;
            f[k] = rc[k].y;
            if (q < a.D) a.groups[q] = rc[k].z;
        }
    } else {
#pragma unroll
        for (uint32_t k = 0; k < INBOX_TILE / INBOX_BLOCK; ++k) {
            const bool ok = j[k] < a.m;
            p[k] = ok ? a.pub_of[j[k]] : NONE;
            f[k] = ok ? a.ids[j[k]] : NONE;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < INBOX_TILE / INBOX_BLOCK; ++k) {
        const uint64_t q = tbase + k * INBOX_BLOCK + t;
        if (q < a.D) {
            a.publishes[q] = p[k];
            a.filter_ids[q] = f[k];
        }
        heads += (uint32_t)__popcll(__ballot(q < a.D && ky[k] != kp[k]));
    }
    if ((t & 63) == 0) hw[t >> 6] = heads;
    __syncthreads();
    if (t == 0) a.hcount[blockIdx.x] = hw[0] + hw[1] + hw[2] + hw[3];
}

// Compaction of the heads: subscribers[r] and inbox_offsets[r] of the r-th
// inbox, r = heads before it (earlier tiles: the scan; earlier waves; earlier
// rounds; lower lanes).
__global__ __launch_bounds__(INBOX_BLOCK) void tm_inbox_heads(InboxArgs a, const uint32_t* keys) {
    __shared__ uint32_t hw[INBOX_BLOCK / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * INBOX_TILE + (uint64_t)w * INBOX_WAVE_PAIRS;
    uint32_t ky[INBOX_ROUNDS];
    uint64_t hm[INBOX_ROUNDS];
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        ky[r] = q < a.D ? keys[q] : 0u;
        const uint32_t kp = (q < a.D && q) ? keys[q - 1] : ~ky[r];
        hm[r] = __ballot(q < a.D && ky[r] != kp);
        mine += (uint32_t)__popcll(hm[r]);
    }
    if (lane == 0) hw[w] = mine;
    __syncthreads();
    uint32_t base = a.hcount[blockIdx.x] + a.hcbs[blockIdx.x / SCAN_TILE];
    for (uint32_t k = 0; k < w; ++k) base += hw[k];
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        if ((hm[r] >> lane) & 1ull) {
            const uint32_t i = base + inbox_mbcnt(hm[r]);
            if (i < a.rcap) {
                a.subscribers[i] = ky[r];
                a.inbox_offsets[i] = (uint32_t)q;
            }
        }
        base += (uint32_t)__popcll(hm[r]);
    }
    if (blockIdx.x == 0 && t == 0) {
        const uint32_t R = *a.d_R;
        if (R <= a.rcap) a.inbox_offsets[R] = a.D;
    }
}

// ------------------------------------- what the session sends (tm_batch_deliver)
//
// emqx_channel:ignore_local/3 (src/emqx_channel.erl:682-693) and
// emqx_session:enrich_subopts/3 (src/emqx_session.erl:500-529) over the
// batch's inboxes.  The kernels walk the deliveries in the sort's tiles (wave
// w of tile t owns pairs [4096 t + 1024 w, + 1024), 64 consecutive pairs per
// round), so a delivery's inbox index is a count of the inbox heads before it:
// the finish's scanned per-tile head counts, the earlier waves of the tile
// (LDS), the earlier rounds and the lower lanes (ballots).
//   range    one search of the table's subscribers per inbox
//   flags    per delivery: its options (a search inside the inbox's range),
//            the enriched byte, own / not own; per inbox the first delivery
//            that is not own (atomicMin, at most one per inbox and wave round,
//            skipped when the minimum read beforehand is lower already: a '#'
//            subscriber's inbox spans thousands of waves)
//   count    keep = not own, or (default mode) behind the inbox's first not-own
//            delivery; that delivery is the head of what is left of the inbox
//   scans    deliveries and heads left per tile (the project's two-level scan)
//   scatter  the stable compaction
// No kernel waits for another workgroup.

// Heads among the wave's pairs -> hw[wave]; returns the heads before the wave's
// first pair.  Every thread of the block calls it.
__device__ __forceinline__ uint32_t dlv_heads_before(const DeliverArgs& a, uint32_t* hw, uint64_t wbase) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const bool on = q < a.D;
        const uint32_t ky = on ? a.keys[q] : 0u;
        const uint32_t kp = (on && q) ? a.keys[q - 1] : ~ky;
        mine += (uint32_t)__popcll(__ballot(on && ky != kp));
    }
    if (lane == 0) hw[w] = mine;
    __syncthreads();
    uint32_t base = a.hcount[blockIdx.x] + a.hcbs[blockIdx.x / SCAN_TILE];
    for (uint32_t k = 0; k < w; ++k) base += hw[k];
    return base;
}

__global__ __launch_bounds__(256) void tm_deliver_range(DeliverArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const uint32_t S = a.subscribers[r];
    uint32_t lo = 0, hi = a.NS;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.tsub[mid] < S) lo = mid + 1; else hi = mid;
    }
    uint2 g = make_uint2(0u, 0u);
    if (lo < a.NS && a.tsub[lo] == S) {
        g.y = min(a.tstart[lo + 1], a.T);
        g.x = min(a.tstart[lo], g.y);
    } else if (!a.groups) {
        atomicAdd(a.err, 1u);   // a subscriber of the fan-out without options: TM_EIO
    }   // armed batch: a member without options is legal; tm_deliver_flags decides per delivery
    a.rng[r] = g;
    a.first[r] = NONE;
}

// GRP (an armed batch): a shared delivery whose (subscriber, filter) has no
// options passes through -- get_subopts/2 gives [] and enrich_subopts([], Msg, _)
// leaves the message alone (src/emqx_session.erl:500-509): the publish's QoS
// and retain flag, no TM_MSG_NL, subid 0, never own.
template <bool DROP, bool GRP>
__global__ __launch_bounds__(INBOX_BLOCK) void tm_deliver_flags(DeliverArgs a) {
    __shared__ uint32_t hw[INBOX_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * INBOX_TILE + (uint64_t)w * INBOX_WAVE_PAIRS;
    uint32_t hb = dlv_heads_before(a, hw, wbase);
    const bool upgrade = a.flags & DLV_UPGRADE_QOS;
    uint32_t bad = 0;
#pragma unroll 2
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const bool on = q < a.D;
        const uint32_t S = on ? a.keys[q] : 0u;
        const uint32_t kp = (on && q) ? a.keys[q - 1] : ~S;
        const uint64_t hm = __ballot(on && S != kp);
        // heads at or before me, less one
        const uint32_t ri = hb + inbox_mbcnt(hm) + (uint32_t)((hm >> lane) & 1ull) - 1u;
        hb += (uint32_t)__popcll(hm);
        bool ok = on && ri < a.R;
        bool pass = false;
        uint32_t v = 0, p = NONE;
        if (ok) {
            p = a.publishes[q];
            const uint32_t f = a.filter_ids[q];
            const uint2 g = a.rng[ri];
            uint32_t lo = g.x, hi = min(g.y, a.T);
            const uint32_t end = hi;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.tnode[mid] < f) lo = mid + 1; else hi = mid;
            }
            if (lo < end && a.tnode[lo] == f) v = a.tval[lo];
            else if (GRP && a.groups[q] != NONE) pass = true;
            else ok = false;
            if (p >= a.n) ok = false;
        }
        if (on && !ok) ++bad;
        const uint32_t pm = (ok && a.msg) ? a.msg[p] : 0u;
        const uint32_t sq = v & SO_QOS, pq = pm & MSG_QOS;
        const uint32_t qos = pass ? pq : upgrade ? max(sq, pq) : min(sq, pq);
        const bool retain = (pm & MSG_RETAIN) && (pass || (v & SO_RAP) || (pm & MSG_RETAINED));
        if (on) {
            a.emsg[q] = (uint8_t)(qos | (retain ? MSG_RETAIN : 0u) | ((v & SO_NL) ? MSG_NL : 0u));
            if (a.esubid) a.esubid[q] = v >> SO_SUBID_SHIFT;
        }
        if (DROP) {
            const uint32_t fr = (ok && a.from) ? a.from[p] : NONE;
            const bool own = ok && (v & SO_NL) && fr != NONE && fr == S;
            if (on) a.own[q] = own ? 1 : 0;
            // the first not-own delivery of my inbox inside this round: no
            // not-own lane between my inbox's first lane of the round and me
            const bool cand = ok && !own;
            const uint64_t nz = __ballot(cand);
            const uint64_t upto = ~0ull >> (63u - lane);   // lanes 0 .. lane
            const uint32_t s = 63u - (uint32_t)__clzll((hm | 1ull) & upto);
            const uint64_t before = nz & (upto >> 1) & ~((1ull << s) - 1ull);
            if (cand && !before) {
                uint32_t* slot = a.first + ri;
                if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)q)
                    atomicMin(slot, (uint32_t)q);
            }
        }
    }
    if (bad) atomicAdd(a.err, bad);
}

__global__ __launch_bounds__(INBOX_BLOCK) void tm_deliver_count(DeliverArgs a) {
    __shared__ uint32_t hw[INBOX_BLOCK / 64], kw[INBOX_BLOCK / 64], nw[INBOX_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * INBOX_TILE + (uint64_t)w * INBOX_WAVE_PAIRS;
    uint32_t hb = dlv_heads_before(a, hw, wbase);
    const bool all = a.flags & DLV_NL_ALL;
    uint32_t kept = 0, heads = 0;
#pragma unroll 2
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const bool on = q < a.D;
        const uint32_t S = on ? a.keys[q] : 0u;
        const uint32_t kp = (on && q) ? a.keys[q - 1] : ~S;
        const uint64_t hm = __ballot(on && S != kp);
        const uint32_t ri = hb + inbox_mbcnt(hm) + (uint32_t)((hm >> lane) & 1ull) - 1u;
        hb += (uint32_t)__popcll(hm);
        const bool ok = on && ri < a.R;
        const uint32_t fst = ok ? a.first[ri] : NONE;
        const bool own = ok && a.own[q];
        const bool keep = ok && (!own || (!all && (uint32_t)q > fst));
        const bool head = keep && (uint32_t)q == fst;
        if (on) a.own[q] = (uint8_t)((keep ? DLV_KEEP : 0) | (head ? DLV_HEAD : 0));
        kept += (uint32_t)__popcll(__ballot(keep));
        heads += (uint32_t)__popcll(__ballot(head));
    }
    if (lane == 0) { kw[w] = kept; nw[w] = heads; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.kcount[blockIdx.x] = kw[0] + kw[1] + kw[2] + kw[3];
        a.ncount[blockIdx.x] = nw[0] + nw[1] + nw[2] + nw[3];
    }
}
static_assert(INBOX_BLOCK / 64 == 4, "four waves per tile");

template <bool GRP>
__global__ __launch_bounds__(INBOX_BLOCK) void tm_deliver_scatter(DeliverArgs a) {
    __shared__ uint32_t kw[INBOX_BLOCK / 64], nw[INBOX_BLOCK / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t wbase = (uint64_t)blockIdx.x * INBOX_TILE + (uint64_t)w * INBOX_WAVE_PAIRS;
    uint32_t kept = 0, heads = 0;
    // (both loops stay short of fully unrolled: seventeen pointers are live, and
    // unrolled further the kernel spills SGPRs)
#pragma unroll 4
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const uint32_t fl = q < a.D ? a.own[q] : 0u;
        kept += (uint32_t)__popcll(__ballot(fl & DLV_KEEP));
        heads += (uint32_t)__popcll(__ballot(fl & DLV_HEAD));
    }
    if (lane == 0) { kw[w] = kept; nw[w] = heads; }
    __syncthreads();
    uint32_t kb = a.kcount[blockIdx.x] + a.kbs[blockIdx.x / SCAN_TILE];
    uint32_t nb = a.ncount[blockIdx.x] + a.nbs[blockIdx.x / SCAN_TILE];
    for (uint32_t k = 0; k < w; ++k) { kb += kw[k]; nb += nw[k]; }
#pragma unroll 1
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const uint32_t fl = q < a.D ? a.own[q] : 0u;
        const uint64_t km = __ballot(fl & DLV_KEEP), hm = __ballot(fl & DLV_HEAD);
        if (fl & DLV_KEEP) {
            const uint32_t pos = kb + inbox_mbcnt(km);
            if (pos < a.D) {
                a.o_pub[pos] = a.publishes[q];
                a.o_fid[pos] = a.filter_ids[q];
                a.o_msg[pos] = a.emsg[q];
                if (a.o_subid) a.o_subid[pos] = a.esubid[q];
                if (GRP) a.o_grp[pos] = a.groups[q];
                if (fl & DLV_HEAD) {
                    const uint32_t i = nb + inbox_mbcnt(hm);
                    if (i < a.R) {
                        a.o_sub[i] = a.keys[q];
                        a.o_off[i] = pos;
                    }
                }
            }
        }
        kb += (uint32_t)__popcll(km);
        nb += (uint32_t)__popcll(hm);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint32_t left = a.d_tot[1];
        if (left <= a.R) a.o_off[left] = a.d_tot[0];
    }
}

// ------------------------------------- the session's send window (tm_batch_window)
//
// emqx_session:deliver/2 (src/emqx_session.erl:421-457) and enqueue/2
// (:459-472) with emqx_mqueue:in/2 (src/emqx_mqueue.erl:148-168) over what
// tm_batch_deliver left.  The reference folds over an inbox; here a delivery's
// outcome follows from its rank among the inbox's *counted* deliveries (QoS > 0
// in a connected inbox, "enters the queue" in a disconnected one) and from the
// inbox's total of them.  Same tiles as the deliver kernels: wave w of tile t
// owns deliveries [4096 t + 1024 w, + 1024), 64 per round.
//   state     per inbox: one search of the uploaded session table (or the
//             defaults), and the inbox's bit in `heads` (one atomicOr per inbox
//             on a word of 32 deliveries; none on the deliveries of an inbox)
//   count     per wave: its counted deliveries; the lane on an inbox head
//             stores the wave's count before it
//   scan      the waves' counts (the project's two-level scan).  Per wave, not
//             per tile: a head's base is then scanned[its wave] + its stored
//             count with no second pass over the tile and no barrier
//   plan      per inbox: base, total (the next head's base, or the grand
//             total), the closed form of the fold -> the inbox's record and
//             the two rank thresholds
//   classify  per delivery: rank = scanned position - base -> disp, packet id;
//             per-wave disposition counts, summed by tm_window_totals
// No kernel waits for another workgroup.

// the heads before the wave's first delivery: off[r] < wbase, r < R
__device__ __forceinline__ uint32_t win_heads_before(const WindowArgs& a, uint32_t wbase) {
    uint32_t lo = 0, hi = a.R;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.off[mid] < wbase) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint64_t win_head_mask(const WindowArgs& a, uint64_t q0) {   // q0: the round's first delivery
    if (q0 >= a.D) return 0ull;
    const uint64_t i = (q0 >> 6) * 2;
    return (uint64_t)a.heads[i] | (uint64_t)a.heads[i + 1] << 32;
}
__device__ __forceinline__ bool win_counted(uint32_t flags, uint32_t qos) {
    if (flags & WIN_HOST) return false;
    return qos > 0 || (flags & (WIN_DISCONNECTED | WIN_STORE_QOS0)) == (WIN_DISCONNECTED | WIN_STORE_QOS0);
}
__device__ __forceinline__ uint32_t win_scanned(const WindowArgs& a, uint32_t gw) {
    return a.wcount[gw] + a.wbs[gw / SCAN_TILE];
}

__global__ __launch_bounds__(256) void tm_window_state(WindowArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const uint32_t S = a.subscribers[r];
    uint32_t lo = 0, hi = a.NS;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.sess[(uint64_t)mid * WIN_SESSION_WORDS] < S) lo = mid + 1; else hi = mid;
    }
    uint4 s;
    if (lo < a.NS && a.sess[(uint64_t)lo * WIN_SESSION_WORDS] == S) {
        const uint32_t* e = a.sess + (uint64_t)lo * WIN_SESSION_WORDS;
        s = make_uint4((e[1] & 0xFFFFu) | (e[2] & WIN_FLAGS) << 16, e[3], e[4], e[5]);
    } else {
        s = make_uint4((a.dflt[1] & 0xFFFFu) | (a.dflt[2] & WIN_FLAGS) << 16, a.dflt[3], a.dflt[4], a.dflt[5]);
    }
    a.st[r] = s;
    const uint32_t o = a.off[r];
    if (o < a.D) atomicOr(a.heads + (o >> 5), 1u << (o & 31u));
    else atomicAdd(a.d_tot + 1, 1u);
}

__global__ __launch_bounds__(INBOX_BLOCK) void tm_window_count(WindowArgs a) {
    const uint32_t lane = threadIdx.x & 63, gw = blockIdx.x * (INBOX_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t wbase = (uint64_t)gw * INBOX_WAVE_PAIRS;
    if (gw >= a.nwaves) return;
    if (wbase >= a.D) {
        if (lane == 0) a.wcount[gw] = 0;
        return;
    }
    uint32_t hb = win_heads_before(a, (uint32_t)wbase);
    uint32_t run = 0, bad = 0;
#pragma unroll 2
    for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
        const uint64_t q = wbase + r * 64 + lane;
        const bool on = q < a.D;
        const uint64_t hm = win_head_mask(a, wbase + r * 64);
        const bool head = (hm >> lane) & 1ull;
        const uint32_t ri = hb + inbox_mbcnt(hm) + (head ? 1u : 0u) - 1u;   // heads at or before me, less one
        hb += (uint32_t)__popcll(hm);
        const bool ok = on && ri < a.R;
        if (on && !ok) ++bad;
        const uint32_t flags = ok ? a.st[ri].x >> 16 : WIN_HOST;
        const uint32_t qos = ok ? a.msg[q] & MSG_QOS : 0u;
        const uint64_t cm = __ballot(ok && win_counted(flags, qos));
        if (ok && head) a.hbase[ri] = run + inbox_mbcnt(cm);
        run += (uint32_t)__popcll(cm);
    }
    if (lane == 0) a.wcount[gw] = run;
    if (bad) atomicAdd(a.d_tot + 1, bad);
}

__global__ __launch_bounds__(256) void tm_window_plan(WindowArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const uint32_t o = a.off[r], on = r + 1 < a.R ? a.off[r + 1] : a.D;
    if (o >= a.D || on > a.D || on <= o) {   // tm_window_state counted it; nothing of this inbox is classified
        a.st[r] = make_uint4(WIN_HOST << 16, 0u, 0u, 0u);
        a.rec[r] = make_uint4(0u, 0u, 0u, 0u);
        if (o < a.D) atomicAdd(a.d_tot + 1, 1u);
        return;
    }
    const uint32_t base = win_scanned(a, o / INBOX_WAVE_PAIRS) + a.hbase[r];
    const uint32_t next = r + 1 < a.R ? win_scanned(a, on / INBOX_WAVE_PAIRS) + a.hbase[r + 1] : a.d_tot[0];
    const uint32_t tot = next - base;   // counted deliveries of the inbox
    const uint4 s = a.st[r];
    const uint32_t P = s.x & 0xFFFFu, flags = s.x >> 16, F = s.y, L = s.z, M = s.w;
    if (flags & WIN_HOST) {
        a.st[r] = make_uint4(s.x, base, 0u, 0u);
        a.rec[r] = make_uint4(P, 0u, 0u, 0u);
        return;
    }
    const uint32_t nsend = (flags & WIN_DISCONNECTED) ? 0u : min(F, tot);
    const uint32_t E = tot - nsend;   // deliveries that enter the queue
    const uint64_t over = (uint64_t)L + E;
    const uint64_t drops = (M && over > M) ? over - M : 0ull;
    const uint32_t dold = (uint32_t)min<uint64_t>(drops, L);
    const uint32_t dnew = (uint32_t)min<uint64_t>(drops - dold, E);
    a.st[r] = make_uint4(s.x, base, nsend, nsend + dnew);
    a.rec[r] = make_uint4((P - 1u + nsend % 65535u) % 65535u + 1u, nsend, E - dnew, dold);
}

__global__ __launch_bounds__(INBOX_BLOCK) void tm_window_classify(WindowArgs a) {
    const uint32_t lane = threadIdx.x & 63, gw = blockIdx.x * (INBOX_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t wbase = (uint64_t)gw * INBOX_WAVE_PAIRS;
    if (gw >= a.nwaves) return;
    uint32_t tot[WIN_NDISP] = {};
    if (wbase < a.D) {
        uint32_t hb = win_heads_before(a, (uint32_t)wbase);
        uint32_t run = win_scanned(a, gw), bad = 0;
#pragma unroll 2
        for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
            const uint64_t q = wbase + r * 64 + lane;
            const bool on = q < a.D;
            const uint64_t hm = win_head_mask(a, wbase + r * 64);
            const uint32_t ri = hb + inbox_mbcnt(hm) + (uint32_t)((hm >> lane) & 1ull) - 1u;
            hb += (uint32_t)__popcll(hm);
            const bool ok = on && ri < a.R;
            if (on && !ok) ++bad;
            const uint4 pl = ok ? a.st[ri] : make_uint4(WIN_HOST << 16, 0u, 0u, 0u);
            const uint32_t P = pl.x & 0xFFFFu, flags = pl.x >> 16;
            const uint32_t qos = ok ? a.msg[q] & MSG_QOS : 0u;
            const bool counted = ok && win_counted(flags, qos);
            const uint64_t cm = __ballot(counted);
            const uint32_t rank = run + inbox_mbcnt(cm) - pl.y;
            run += (uint32_t)__popcll(cm);
            uint32_t d, id = 0;
            if (flags & WIN_HOST) d = 5u;                                   // TM_DISP_HOST
            else if (!counted) d = (flags & WIN_DISCONNECTED) ? 3u : 0u;    // TM_DISP_DROP_QOS0 : TM_DISP_SEND0
            else if (rank < pl.z) { d = 1u; id = (P - 1u + rank % 65535u) % 65535u + 1u; }   // TM_DISP_SEND
            else d = rank < pl.w ? 4u : 2u;                                 // TM_DISP_DROP_FULL : TM_DISP_QUEUED
            if (on) {
                a.disp[q] = (uint8_t)d;
                a.pid[q] = (uint16_t)id;
            }
#pragma unroll
            for (uint32_t k = 0; k < WIN_NDISP; ++k) tot[k] += (uint32_t)__popcll(__ballot(on && d == k));
        }
        if (bad) atomicAdd(a.d_tot + 1, bad);
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < WIN_NDISP; ++k) a.wdisp[(uint64_t)gw * 8 + k] = tot[k];
    }
}
static_assert(WIN_NDISP <= 8, "a wave's disposition counts fit its eight words");

// the waves' disposition counts -> totals (one block), as tm_stats_reduce sums the walk's
__global__ __launch_bounds__(256) void tm_window_totals(WindowArgs a) {
    __shared__ unsigned long long sh[4][WIN_NDISP];
    unsigned long long v[WIN_NDISP] = {};
    for (uint32_t i = threadIdx.x; i < a.nwaves; i += 256)
#pragma unroll
        for (uint32_t k = 0; k < WIN_NDISP; ++k) v[k] += a.wdisp[(uint64_t)i * 8 + k];
#pragma unroll
    for (uint32_t k = 0; k < WIN_NDISP; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < WIN_NDISP) {
        const uint32_t k = threadIdx.x;
        a.totals[k] = sh[0][k] + sh[1][k] + sh[2][k] + sh[3][k];
    }
}

// ------------------------------------------ batched predicate (emqx_topic:match/2)

// One thread per name, all rules: the word-by-word clauses of
// emqx_topic:match/2 (src/emqx_topic.erl:74-87) -- equal words or a '+' rule
// word advance, a trailing '#' matches the rest (zero words included), both
// exhausted matches -- plus the binary form's '$' rule (:68-71) when asked.
// Rule words are read by every thread at once (broadcast, L1/L2-resident).
__global__ __launch_bounds__(256) void tm_rules_match(RulesArgs a) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n) return;
    const uint32_t nb = a.noff[t], nl = a.noff[t + 1] - nb;
    const bool dollar = a.dollar_rule && (a.nflag[t] & 1);
    for (uint32_t w0 = 0; w0 < a.r; w0 += 32) {
        uint32_t acc = 0;
        const uint32_t w1 = min(a.r, w0 + 32);
        for (uint32_t j = w0; j < w1; ++j) {
            const uint32_t rb = a.roff[j], rl = a.roff[j + 1] - rb;
            bool m = false;
            if (!(dollar && (a.rflag[j] & 1))) {
                uint32_t i = 0, k = 0;
                for (;;) {
                    if (i == nl && k == rl) { m = true; break; }
                    const uint32_t fw = k < rl ? a.rwords[rb + k] : 0u;
                    // [H|T1] against [H|T2] is tried before (_, ['#']): a name's own '#' is consumed
                    if (i < nl && k < rl && (fw == W_PLUS || fw == a.nwords[nb + i])) { ++i; ++k; continue; }
                    m = k + 1 == rl && fw == W_HASH;
                    break;
                }
            }
            acc |= (uint32_t)m << (j - w0);
        }
        a.bits[(uint64_t)t * a.wpr + w0 / 32] = acc;
    }
}

// ------------------------------------------------ batched ACL check (tm_acl_check)

// a >= b over four big-endian words (an address in network order)
__device__ __forceinline__ bool acl_ip_ge(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t b0,
                                          uint32_t b1, uint32_t b2, uint32_t b3) {
    return a0 != b0 ? a0 > b0 : a1 != b1 ? a1 > b1 : a2 != b2 ? a2 > b2 : a3 >= b3;
}

// match_who/2 (src/emqx_access_rule.erl:101-124) of client c over the rule's
// postfix program blk[pc .. pe): every lane of the wave runs the same ops
// (uniform reads), only the client's bytes differ per lane.
__device__ __forceinline__ bool acl_who(const AclArgs& a, const uint8_t* bb, uint32_t pc, uint32_t pe, uint32_t c,
                                        uint32_t cf) {
    uint32_t st = 0;
    while (pc < pe) {
        const uint32_t w = a.blk[pc], op = w & 15u, arg = w >> 4;
        if (op == ACL_OP_TRUE || op == ACL_OP_FALSE) {
            st = (st << 1) | (op == ACL_OP_TRUE ? 1u : 0u);
            pc += 1;
        } else if (op == ACL_OP_CLIENT || op == ACL_OP_USER) {
            // binary equality; an undefined field equals no binary (:107-110)
            const bool isc = op == ACL_OP_CLIENT;
            const uint8_t* v = bb + a.blk[pc + 1];
            bool ok = (cf & (isc ? 1u : 2u)) != 0;
            if (ok) {
                const uint64_t* off = isc ? a.cid_off : a.usr_off;
                const uint64_t o = off[c], l = off[c + 1] - o;
                const uint8_t* p = (isc ? a.cid : a.usr) + o;
                ok = l == arg;
                for (uint32_t i = 0; ok && i < arg; ++i) ok = p[i] == v[i];
            }
            st = (st << 1) | (ok ? 1u : 0u);
            pc += 2;
        } else if (op == ACL_OP_IPADDR) {
            // Start =< IP =< End within one family; peerhost undefined -> false (:111-114)
            bool ok = a.cfamily[c] == arg;
            if (ok) {
                const uint4 q = a.peer[c];
                const uint32_t i0 = __builtin_bswap32(q.x), i1 = __builtin_bswap32(q.y), i2 = __builtin_bswap32(q.z),
                               i3 = __builtin_bswap32(q.w);
                ok = acl_ip_ge(i0, i1, i2, i3, a.blk[pc + 1], a.blk[pc + 2], a.blk[pc + 3], a.blk[pc + 4]) &&
                     acl_ip_ge(a.blk[pc + 5], a.blk[pc + 6], a.blk[pc + 7], a.blk[pc + 8], i0, i1, i2, i3);
            }
            st = (st << 1) | (ok ? 1u : 0u);
            pc += 9;
        } else {   // AND / OR: fold the child on top into the accumulator below it (:115-122)
            const uint32_t b = st & 1u;
            st >>= 1;
            st = op == ACL_OP_AND ? (st & (~1u | b)) : (st | b);
            pc += 1;
        }
    }
    return (st & 1u) != 0;
}

// One lane = one request, the rules in list order: the access mask
// (emqx_mod_acl_internal:filter/2, src/emqx_mod_acl_internal.erl:110-121), the
// who program, then the name's bytes against each filter level by level --
// emqx_topic:match/2 on word lists (src/emqx_topic.erl:74-87: an equal word or
// a '+' filter word advances, a last '#' takes the rest, both exhausted
// match; no '$' rule), where a level is a word and words compare as bytes
// except that a %c / %u level holding the client's id / name (feed_var,
// src/emqx_access_rule.erl:141-154) is a binary and so never equals the atoms
// '' / '+' / '#' of the name.  {eq, T} is byte equality of the whole topic.
// The first matching rule decides (src/emqx_mod_acl_internal.erl:82-90); the
// wave leaves the rule loop once every lane has decided.  LDS: the block's
// names were staged into sm (name bytes at sm + (o - a0)); otherwise they are
// read from global memory.
template <bool LDS>
__device__ __forceinline__ void acl_lane(const AclArgs& a, const uint8_t* sm, uint64_t a0, uint32_t t) {
    const bool active = t < a.n;
    uint32_t nlen = 0, c = 0, acc = 0, cf = 0;
    uint64_t o = a0;
    if (active) {
        o = a.offs[t] - a.base;
        nlen = (uint32_t)(a.offs[t + 1] - a.offs[t]);
        c = a.client_of[t];
        acc = a.access[t];
        cf = a.cflags[c];
    }
    const uint8_t* ns = sm + (uint32_t)(o - a0);
    const uint8_t* ng = a.topics + o;
    auto nb = [&](uint32_t i) -> uint32_t { return LDS ? ns[i] : ng[i]; };
    // the name level at pos is exactly the l bytes at p (a level holds no '/':
    // a client id with one is one word and equals no level)
    auto level_is = [&](uint32_t pos, const uint8_t* p, uint32_t l) -> bool {
        if (pos + l > nlen) return false;
        if (pos + l < nlen && nb(pos + l) != '/') return false;
        for (uint32_t i = 0; i < l; ++i) {
            const uint32_t b = p[i];
            if (b == '/' || nb(pos + i) != b) return false;
        }
        return true;
    };
    const uint8_t* bb = reinterpret_cast<const uint8_t*>(a.blk);
    uint32_t verdict = ACL_NOMATCH, rule = NONE;
    bool decided = !active;
    for (uint32_t j = 0; j < a.n_rules; ++j) {
        if (__ballot(!decided) == 0ull) break;
        const uint32_t* rw = a.blk + ACL_HDR + ACL_RULE_W * j;
        const uint32_t flags = rw[0];
        if (decided) continue;
        bool m = (flags >> 16) & 1u;                       // {A, all}
        if (!m && (((flags >> 8) & 3u) & acc) && acl_who(a, bb, rw[1], rw[1] + rw[2], c, cf)) {
            const uint32_t ntop = rw[4];
            for (uint32_t f = 0; f < ntop && !m; ++f) {
                const uint32_t* tw = a.blk + rw[3] + ACL_TOPIC_W * f;
                const uint8_t* fb = bb + tw[0];
                const uint32_t flen = tw[1] & ~ACL_EQ;
                if (tw[1] & ACL_EQ) {
                    m = flen == nlen;
                    for (uint32_t i = 0; m && i < flen; ++i) m = nb(i) == fb[i];
                    continue;
                }
                const uint32_t nlev = tw[3];
                uint32_t pos = 0;
                bool have = true;                          // the name has a level at pos
                bool done = false;
                for (uint32_t k = 0; k < nlev; ++k) {
                    const uint32_t lv = a.blk[tw[2] + k];
                    const uint32_t kind = (lv >> ACL_L_KIND_SHIFT) & 7u;
                    uint32_t l = (lv >> ACL_L_LEN_SHIFT) & ACL_L_MASK;
                    const uint8_t* p = fb + (lv & ACL_L_MASK);
                    bool adv = false;
                    if (have) {
                        if (kind == ACL_L_PLUS) {
                            uint32_t e = pos;
                            while (e < nlen && nb(e) != '/') ++e;
                            l = e - pos;
                            adv = true;
                        } else {
                            bool ok = true;
                            const bool vc = kind == ACL_L_VARC && (cf & 1u), vu = kind == ACL_L_VARU && (cf & 2u);
                            if (vc || vu) {
                                const uint64_t* off = vc ? a.cid_off : a.usr_off;
                                const uint64_t vo = off[c], vl = off[c + 1] - vo;
                                p = (vc ? a.cid : a.usr) + vo;
                                l = (uint32_t)(vl < 0xFFFFull ? vl : 0xFFFFull);
                                // the name's '' / '+' / '#' levels are atoms, the value a binary
                                ok = l > 1u || (l == 1u && p[0] != '+' && p[0] != '#');
                            }
                            adv = ok && level_is(pos, p, l);
                        }
                    }
                    if (adv) {
                        if (pos + l == nlen) have = false;
                        else pos += l + 1u;
                        continue;
                    }
                    m = kind == ACL_L_HASH && (lv & ACL_L_LAST);
                    done = true;
                    break;
                }
                if (!done) m = !have;
            }
        }
        if (m) {
            decided = true;
            verdict = flags & 1u;
            rule = j;
        }
    }
    if (active) {
        a.verdict[t] = (uint8_t)verdict;
        a.rule[t] = rule;
    }
}

__global__ __launch_bounds__(256) void tm_acl_check(AclArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t sm[ACL_STAGE + 16];
    const uint32_t t0 = blockIdx.x * 256u, t1 = min(a.n, t0 + 256u);
    // the block's names are one contiguous byte range
    const uint64_t b0 = a.offs[t0] - a.base, b1 = a.offs[t1] - a.base;
    const uint64_t a0 = b0 & ~15ull;
    if (b1 - a0 <= ACL_STAGE) {
        const uint32_t nv = (uint32_t)((b1 - a0 + 15u) >> 4);
        const uint4* src = reinterpret_cast<const uint4*>(a.topics + a0);
        uint4* dst = reinterpret_cast<uint4*>(sm);
        for (uint32_t i = threadIdx.x; i < nv; i += 256u) dst[i] = src[i];
        __syncthreads();
        acl_lane<true>(a, sm, a0, t0 + threadIdx.x);
    } else {
        acl_lane<false>(a, sm, a0, t0 + threadIdx.x);
    }
}

// ------------------------------------------------ device dedup (TM_BATCH_DEDUP)

// 8 bytes at byte offset s of a 4-aligned LDS array (any alignment of s)
__device__ __forceinline__ uint64_t lds_u64(const uint8_t* base, uint32_t s) {
    const uint32_t a = s & ~3u, sh = (s & 3u) * 8u;
    const uint32_t d0 = *reinterpret_cast<const uint32_t*>(base + a);
    const uint32_t d1 = *reinterpret_cast<const uint32_t*>(base + a + 4);
    const uint32_t d2 = *reinterpret_cast<const uint32_t*>(base + a + 8);
    const uint64_t lo = ((uint64_t)d1 << 32) | d0;
    return sh ? (lo >> sh) | ((uint64_t)d2 << (64u - sh)) : lo;
}

__device__ __forceinline__ uint64_t low_bytes(uint64_t v, uint32_t k) {   // first k (< 8) bytes of v
    return k >= 8 ? v : (v & ((1ull << (8u * k)) - 1ull));
}



// A topic's first 64 bytes as 16 little-endian u32 words, zero past len:
// the 16-B aligned loads that cover them (the batch bytes are 16-B aligned
// and padded by 16), all issued before any is used, then the topic's offset
// within the first load taken out in 32-bit ops only -- two word selects and
// one v_alignbyte per word (64-bit variable shifts cost 3-4 VALU each).
// Lanes of a wave read neighbouring topics, so a load instruction's lines are
// mostly the wave's next ones.
__device__ __forceinline__ void dd_load64(const uint8_t* bytes, uint64_t b, uint32_t len, uint32_t (&c)[16]) {
    const uint64_t a0 = b & ~15ull;
    const uint32_t sh = (uint32_t)(b & 15u);
    const uint32_t need = sh + (len < 64u ? len : 64u);
    uint32_t w[20];
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (16u * k < need) v = *reinterpret_cast<const uint4*>(bytes + a0 + 16u * k);
        w[4 * k] = v.x;
        w[4 * k + 1] = v.y;
        w[4 * k + 2] = v.z;
        w[4 * k + 3] = v.w;
    }
    // (selects as masks: written as `q ? w[i + 1] : w[i]` the compiler turns
    // them into one dynamically indexed array -- scratch memory)
    const uint32_t m1 = 0u - ((sh >> 2) & 1u), m2 = 0u - ((sh >> 3) & 1u);
    uint32_t s1[19];
#pragma unroll
    for (uint32_t i = 0; i < 19; ++i) s1[i] = w[i] ^ ((w[i] ^ w[i + 1]) & m1);
    uint32_t s2[17];
#pragma unroll
    for (uint32_t i = 0; i < 17; ++i) s2[i] = s1[i] ^ ((s1[i] ^ s1[i + 2]) & m2);
    const uint32_t r = sh & 3u;
    const uint32_t pm = (1u << ((len & 3u) * 8u)) - 1u;   // the partial last word's bytes
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) {
        const uint32_t x = __builtin_amdgcn_alignbyte(s2[j + 1], s2[j], r);
        c[j] = 4u * j + 4u <= len ? x : (4u * j < len ? (x & pm) : 0u);
    }
}

// 8 bytes at any offset of the padded batch bytes: two aligned 8-B loads and a funnel shift
__device__ __forceinline__ uint64_t dd_u64(const uint8_t* bytes, uint64_t s) {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(bytes + (s & ~7ull));
    const uint32_t sh = (uint32_t)(s & 7u) * 8u;
    const uint64_t lo = q[0];
    return sh ? (lo >> sh) | (q[1] << (64u - sh)) : lo;
}

__device__ __forceinline__ uint64_t dd_mix(uint64_t h, uint64_t c) {
    c *= 0x87C37B91114253D5ull;
    c = (c << 31) | (c >> 33);
    c *= 0x4CF5AD432745937Full;
    h ^= c;
    h = (h << 27) | (h >> 37);
    return h * 5u + 0x52DCE729ull;
}

// 64-bit hash of a topic.  The first 64 bytes: NH (sum over word pairs of
// (w[2i] + k[2i]) * (w[2i+1] + k[2i+1]), exact 32x32 -> 64-bit products: one
// v_mad_u64_u32 per 8 bytes, where a 64x64 multiply chain took three 64-bit
// multiplies of ~4 quarter-rate ops each); the bytes past 64 (rare) chained
// through dd_mix; then the length and a 64-bit finaliser.  Only the table's
// spread depends on it: a collision costs a probe and a byte compare.
__device__ __forceinline__ uint64_t dd_hash(const uint8_t* bytes, uint64_t b, uint32_t len, const uint32_t (&c)[16]) {
    constexpr uint32_t K[16] = {0x9E3779B1u, 0x85EBCA77u, 0xC2B2AE3Du, 0x27D4EB2Fu, 0x165667B1u, 0xD3A2646Du,
                                0xFD7046C5u, 0xB55A4F09u, 0x6C8E9CF5u, 0x7FEB352Du, 0x846CA68Bu, 0x94D049BBu,
                                0xBF58476Du, 0x1CE4E5B9u, 0x2545F491u, 0x9FB21C65u};
    uint64_t h = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) h += (uint64_t)(c[2 * j] + K[2 * j]) * (uint64_t)(c[2 * j + 1] + K[2 * j + 1]);
    for (uint32_t k = 64; k < len; k += 8)   // (topics over 64 bytes: rare, kept narrow)
        h = dd_mix(h, low_bytes(dd_u64(bytes, b + k), len - k < 8u ? len - k : 8u));
    h ^= (uint64_t)len * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 33;
    h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33;
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 33);
}

// the len bytes at b (first 64 in c) equal to the len bytes at ob?
__device__ __forceinline__ bool dd_equal(const uint8_t* bytes, const uint32_t (&c)[16], uint64_t b, uint64_t ob,
                                         uint32_t len) {
    uint32_t o[16];
    dd_load64(bytes, ob, len, o);
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) diff |= c[j] ^ o[j];
    for (uint32_t k = 64; diff == 0 && k < len; k += 8)   // (topics over 64 bytes: rare, kept narrow)
        diff |= low_bytes(dd_u64(bytes, b + k) ^ dd_u64(bytes, ob + k), len - k < 8u ? len - k : 8u) != 0;
    return diff == 0;
}

// ------------------- the send window over priority tables (tm_batch_window_prio)
//
// emqx_mqueue:in/2 with a p_table (src/emqx_mqueue.erl:151-168): Priority =
// get_priority(Topic, PTab, Dp) picks one of the table's classes, and every
// class is a bounded queue of its own.  Which deliveries are sent is the old
// plan's business (the counted rank against nsend); the ENTERING deliveries
// (counted rank >= nsend) of a tabled inbox then need their rank within
// (inbox, class), found the way the window finds the counted rank, per class:
//   lookup    per (table, publish): the class of the publish's topic bytes
//   session   per inbox: its table and its entry of `prio` (one search)
//   count     per wave: its entering deliveries per class, one ballot per
//             class and round; the lane on an inbox head stores the wave's
//             counts before it
//   scan      the waves' counts per class, two levels (tiles of
//             PRIO_SCAN_TILE waves, then the tiles' sums)
//   plan      per inbox: per class base, total, the closed form in 64 bits ->
//             {base, dnew} and the class record; the inbox's record holds
//             the sums
//   classify  per delivery: the old classify, with DROP_FULL / QUEUED of a
//             tabled inbox decided by the class rank; pclass
// An inbox without a table goes through the same kernels and keeps what the
// old plan gave it.  No kernel waits for another workgroup, no thread loops
// over an inbox, no atomics on the deliveries.

// the len bytes at b of `bytes` (first 64 in c) equal to the len bytes at ob of `other`?
__device__ __forceinline__ bool prio_equal(const uint8_t* bytes, const uint32_t (&c)[16], uint64_t b,
                                           const uint8_t* other, uint64_t ob, uint32_t len) {
    uint32_t o[16];
    dd_load64(other, ob, len, o);
    uint32_t diff = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) diff |= c[j] ^ o[j];
    for (uint32_t k = 64; diff == 0 && k < len; k += 8)   // (keys over 64 bytes: rare, kept narrow)
        diff |= low_bytes(dd_u64(bytes, b + k) ^ dd_u64(other, ob + k), len - k < 8u ? len - k : 8u) != 0;
    return diff == 0;
}

// One thread per publish, one grid row per table.  A hash collision costs a
// probe: a slot is accepted only when hash bits, length and bytes all agree.
__global__ __launch_bounds__(256) void tm_prio_lookup(PrioLookupArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
    if (i >= a.n) return;
    const uint32_t* hd = a.blk + PRIO_HDR_W * t;
    const uint2* slots = reinterpret_cast<const uint2*>(a.blk + hd[0]);
    const uint8_t* keys = reinterpret_cast<const uint8_t*>(a.blk) + hd[1];
    const uint32_t mask = hd[2];
    uint32_t cls = hd[3];
    const uint64_t b = a.offs[i] - a.base, l64 = a.offs[i + 1] - a.offs[i];
    if (l64 <= PRIO_MAX_KEY) {   // a longer topic equals no key
        const uint32_t len = (uint32_t)l64;
        uint32_t c[16];
        dd_load64(a.bytes, b, len, c);
        const uint64_t h = dd_hash(a.bytes, b, len, c);
        const uint32_t want = PRIO_META_USED | (uint32_t)(h >> 54) << PRIO_META_HASH_SHIFT | len;
        uint32_t s = (uint32_t)h & mask;
        for (uint32_t k = 0; k <= mask; ++k, s = (s + 1) & mask) {
            const uint2 e = slots[s];
            if (!e.y) break;
            if ((e.y & ~(0xFFu << PRIO_META_CLS_SHIFT)) == want && prio_equal(a.bytes, c, b, keys, e.x, len)) {
                cls = (e.y >> PRIO_META_CLS_SHIFT) & 0xFFu;
                break;
            }
        }
    }
    a.out[(uint64_t)t * a.n + i] = (uint8_t)cls;
}

__global__ __launch_bounds__(256) void tm_winp_session(WindowArgs a, PrioArgs p) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const uint32_t S = a.subscribers[r];
    uint32_t lo = 0, hi = p.NP;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (p.prio[(uint64_t)mid * PRIO_SESSION_WORDS] < S) lo = mid + 1; else hi = mid;
    }
    const uint4 s = a.st[r];   // tm_window_state's {P | flags << 16, F, L, M}
    uint4 g = make_uint4(p.dtab, NONE, s.w, 0u);
    if (lo < p.NP && p.prio[(uint64_t)lo * PRIO_SESSION_WORDS] == S) {
        g.x = p.prio[(uint64_t)lo * PRIO_SESSION_WORDS + 1];
        g.y = lo;
    }
    if (g.x >= p.ntab || ((s.x >> 16) & WIN_HOST)) g.x = g.y = NONE;   // TM_SESS_HOST wins over a table
    p.ptab[r] = g;
}

// the scanned per-class counts before wave gw (after the scan)
__device__ __forceinline__ uint32_t winp_scanned(const PrioArgs& p, uint32_t gw, uint32_t c) {
    return p.cw[(uint64_t)gw * PRIO_CLASSES + c] + p.cbs[(uint64_t)(gw / PRIO_SCAN_TILE) * PRIO_CLASSES + c];
}

// after tm_window_plan: st[r] = {P | flags << 16, base, nsend, .}
__global__ __launch_bounds__(INBOX_BLOCK) void tm_winp_count(WindowArgs a, PrioArgs p) {
    const uint32_t lane = threadIdx.x & 63, gw = blockIdx.x * (INBOX_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t wbase = (uint64_t)gw * INBOX_WAVE_PAIRS;
    if (gw >= a.nwaves) return;
    uint32_t crun[PRIO_CLASSES] = {};
    if (wbase < a.D) {
        uint32_t hb = win_heads_before(a, (uint32_t)wbase);
        uint32_t run = win_scanned(a, gw), bad = 0;
#pragma unroll 1
        for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
            const uint64_t q = wbase + r * 64 + lane;
            const bool on = q < a.D;
            const uint64_t hm = win_head_mask(a, wbase + r * 64);
            const bool head = (hm >> lane) & 1ull;
            const uint32_t ri = hb + inbox_mbcnt(hm) + (head ? 1u : 0u) - 1u;
            hb += (uint32_t)__popcll(hm);
            const bool ok = on && ri < a.R;
            const uint4 pl = ok ? a.st[ri] : make_uint4(WIN_HOST << 16, 0u, 0u, 0u);
            const uint32_t flags = pl.x >> 16;
            const uint32_t qos = ok ? a.msg[q] & MSG_QOS : 0u;
            const bool counted = ok && win_counted(flags, qos);
            const uint64_t cm = __ballot(counted);
            const uint32_t rank = run + inbox_mbcnt(cm) - pl.y;
            run += (uint32_t)__popcll(cm);
            const uint32_t tb = ok ? p.ptab[ri].x : NONE;
            bool ent = counted && rank >= pl.z && tb < p.ntab;
            uint32_t cls = PRIO_NOCLASS;
            if (ent) {
                const uint32_t pub = p.publishes[q];
                if (pub < p.n) cls = p.pcp[(uint64_t)tb * p.n + pub];
                else { ent = false; ++bad; }
            }
            uint32_t hv[PRIO_CLASSES];
#pragma unroll
            for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
                hv[c] = crun[c];
                if (c < p.ncls) {   // (wave-uniform)
                    const uint64_t m = __ballot(ent && cls == c);
                    hv[c] += inbox_mbcnt(m);
                    crun[c] += (uint32_t)__popcll(m);
                }
            }
            if (ok && head) {
                uint4* hbp = reinterpret_cast<uint4*>(p.chbase + (uint64_t)ri * PRIO_CLASSES);
                hbp[0] = make_uint4(hv[0], hv[1], hv[2], hv[3]);
                hbp[1] = make_uint4(hv[4], hv[5], hv[6], hv[7]);
            }
        }
        if (bad) atomicAdd(a.d_tot + 1, bad);
    }
    if (lane == 0) {
        uint4* wp = reinterpret_cast<uint4*>(p.cw + (uint64_t)gw * PRIO_CLASSES);
        wp[0] = make_uint4(crun[0], crun[1], crun[2], crun[3]);
        wp[1] = make_uint4(crun[4], crun[5], crun[6], crun[7]);
    }
}
static_assert(PRIO_CLASSES == 8, "two uint4 per class vector");

// Level one of the class-count scan: a block owns PRIO_SCAN_TILE waves, thread
// (segment sg, class c) 32 of them; exclusive in place, the tile's sums to cbs.
__global__ __launch_bounds__(256) void tm_winp_scan_tiles(PrioArgs p, uint32_t nwaves) {
    __shared__ uint32_t seg[32][PRIO_CLASSES];
    const uint32_t c = threadIdx.x & 7u, sg = threadIdx.x >> 3;
    const uint32_t w0 = blockIdx.x * PRIO_SCAN_TILE + sg * 32u;
    uint32_t sum = 0;
    for (uint32_t i = 0; i < 32u; ++i)
        if (w0 + i < nwaves) sum += p.cw[(uint64_t)(w0 + i) * PRIO_CLASSES + c];
    seg[sg][c] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t k = 0; k < sg; ++k) run += seg[k][c];
    if (sg == 31u) p.cbs[(uint64_t)blockIdx.x * PRIO_CLASSES + c] = run + sum;
    for (uint32_t i = 0; i < 32u; ++i)
        if (w0 + i < nwaves) {
            const uint64_t at = (uint64_t)(w0 + i) * PRIO_CLASSES + c;
            const uint32_t v = p.cw[at];
            p.cw[at] = run;
            run += v;
        }
}
static_assert(PRIO_SCAN_TILE == 32 * 32, "32 segments of 32 waves");

// Level two: the tiles' sums, exclusive in place, and the batch's totals (one
// thread per class; at most 2^32 / (1024 * PRIO_SCAN_TILE) = 4096 tiles).
__global__ __launch_bounds__(64) void tm_winp_scan_sums(PrioArgs p, uint32_t nblocks) {
    const uint32_t c = threadIdx.x;
    if (c >= PRIO_CLASSES) return;
    uint32_t run = 0;
    for (uint32_t k = 0; k < nblocks; ++k) {
        const uint32_t v = p.cbs[(uint64_t)k * PRIO_CLASSES + c];
        p.cbs[(uint64_t)k * PRIO_CLASSES + c] = run;
        run += v;
    }
    p.ctot[c] = run;
}

__global__ __launch_bounds__(256) void tm_winp_plan(WindowArgs a, PrioArgs p) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const uint4 s = a.st[r];   // tm_window_plan's: an inbox it refused is WIN_HOST
    const uint4 g = p.ptab[r];
    uint2* thr = p.cthr + (uint64_t)r * PRIO_CLASSES;
    uint2* rec = p.prec + (uint64_t)r * PRIO_CLASSES;
    if (((s.x >> 16) & WIN_HOST) || g.x >= p.ntab) {
#pragma unroll
        for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
            thr[c] = make_uint2(0u, 0u);
            rec[c] = make_uint2(0u, 0u);
        }
        return;
    }
    const uint32_t o = a.off[r], on = r + 1 < a.R ? a.off[r + 1] : a.D;   // (tm_window_plan checked them)
    const uint32_t wo = o / INBOX_WAVE_PAIRS, wn = on / INBOX_WAVE_PAIRS;
    const bool last = r + 1 >= a.R;
    const uint32_t M = g.z;
    const uint32_t* plen = g.y < p.NP ? p.prio + (uint64_t)g.y * PRIO_SESSION_WORDS + 2 : nullptr;
    uint32_t nq = 0, nold = 0;
#pragma unroll
    for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
        const uint32_t base = winp_scanned(p, wo, c) + p.chbase[(uint64_t)r * PRIO_CLASSES + c];
        const uint32_t next = last ? p.ctot[c] : winp_scanned(p, wn, c) + p.chbase[(uint64_t)(r + 1) * PRIO_CLASSES + c];
        const uint32_t E = next - base;   // entering deliveries of the inbox in class c
        const uint32_t L = plen ? plen[c] : 0u;
        const uint64_t over = (uint64_t)L + E;
        const uint64_t drops = (M && over > M) ? over - M : 0ull;
        const uint32_t dold = (uint32_t)min<uint64_t>(drops, L);
        const uint32_t dnew = (uint32_t)min<uint64_t>(drops - dold, E);
        thr[c] = make_uint2(base, dnew);
        rec[c] = make_uint2(E - dnew, dold);
        nq += E - dnew;
        nold += dold;
    }
    const uint4 old = a.rec[r];   // next_pkt_id and n_inflight do not depend on the queue
    a.rec[r] = make_uint4(old.x, old.y, nq, nold);
}

__global__ __launch_bounds__(INBOX_BLOCK) void tm_winp_classify(WindowArgs a, PrioArgs p) {
    const uint32_t lane = threadIdx.x & 63, gw = blockIdx.x * (INBOX_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t wbase = (uint64_t)gw * INBOX_WAVE_PAIRS;
    if (gw >= a.nwaves) return;
    uint32_t tot[WIN_NDISP] = {};
    if (wbase < a.D) {
        uint32_t crun[PRIO_CLASSES];
#pragma unroll
        for (uint32_t c = 0; c < PRIO_CLASSES; ++c) crun[c] = winp_scanned(p, gw, c);
        uint32_t hb = win_heads_before(a, (uint32_t)wbase);
        uint32_t run = win_scanned(a, gw), bad = 0;
#pragma unroll 1
        for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
            const uint64_t q = wbase + r * 64 + lane;
            const bool on = q < a.D;
            const uint64_t hm = win_head_mask(a, wbase + r * 64);
            const uint32_t ri = hb + inbox_mbcnt(hm) + (uint32_t)((hm >> lane) & 1ull) - 1u;
            hb += (uint32_t)__popcll(hm);
            const bool ok = on && ri < a.R;
            if (on && !ok) ++bad;
            const uint4 pl = ok ? a.st[ri] : make_uint4(WIN_HOST << 16, 0u, 0u, 0u);
            const uint32_t P = pl.x & 0xFFFFu, flags = pl.x >> 16;
            const uint32_t qos = ok ? a.msg[q] & MSG_QOS : 0u;
            const bool counted = ok && win_counted(flags, qos);
            const uint64_t cm = __ballot(counted);
            const uint32_t rank = run + inbox_mbcnt(cm) - pl.y;
            run += (uint32_t)__popcll(cm);
            const uint32_t tb = ok ? p.ptab[ri].x : NONE;
            const bool tabled = tb < p.ntab && !(flags & WIN_HOST);
            uint32_t cls = PRIO_NOCLASS;
            if (tabled) {
                const uint32_t pub = p.publishes[q];
                if (pub < p.n) cls = p.pcp[(uint64_t)tb * p.n + pub];
                else ++bad;
            }
            const bool ent = counted && rank >= pl.z && cls < PRIO_CLASSES;
            uint32_t crank = 0;
#pragma unroll
            for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
                if (c < p.ncls) {   // (wave-uniform)
                    const uint64_t m = __ballot(ent && cls == c);
                    if (cls == c) crank = crun[c] + inbox_mbcnt(m);
                    crun[c] += (uint32_t)__popcll(m);
                }
            }
            uint32_t d, id = 0;
            if (flags & WIN_HOST) d = 5u;                                   // TM_DISP_HOST
            else if (!counted) d = (flags & WIN_DISCONNECTED) ? 3u : 0u;    // TM_DISP_DROP_QOS0 : TM_DISP_SEND0
            else if (rank < pl.z) { d = 1u; id = (P - 1u + rank % 65535u) % 65535u + 1u; }   // TM_DISP_SEND
            else if (ent) {                                                 // the class's own queue
                const uint2 th = p.cthr[(uint64_t)ri * PRIO_CLASSES + cls];
                d = crank - th.x < th.y ? 4u : 2u;
            } else d = rank < pl.w ? 4u : 2u;                               // TM_DISP_DROP_FULL : TM_DISP_QUEUED
            if (on) {
                a.disp[q] = (uint8_t)d;
                a.pid[q] = (uint16_t)id;
                p.pclass[q] = (uint8_t)cls;
            }
#pragma unroll
            for (uint32_t k = 0; k < WIN_NDISP; ++k) tot[k] += (uint32_t)__popcll(__ballot(on && d == k));
        }
        if (bad) atomicAdd(a.d_tot + 1, bad);
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < WIN_NDISP; ++k) a.wdisp[(uint64_t)gw * 8 + k] = tot[k];
    }
}

// ------------------------------------------ the session drain (tm_sessions_drain)
//
// emqx_session:dequeue/1,3 (src/emqx_session.erl:389-413) over the messages a
// batch of sessions holds in its mqueues, each session's listed in arrival
// order.  emqx_mqueue:out/1 pops the highest class first and FIFO within a
// class, so with C(m) = the session's counted messages (not expired, QoS > 0)
// in the classes above m's plus those of m's class before m, m is popped iff
// C(m) < Cnt: the fold has a closed form over per-(session, class) ranks, and
// those are found as the priority window finds its class ranks, here for three
// PLANES at once (counted, QoS 0 not expired, expired).  Same tiles: wave w of
// tile t owns messages [4096 t + 1024 w, + 1024), 64 per round.
//   heads     per session: its bit in `heads` (one atomicOr per session)
//   count     per message: expired? -> kind; per wave and class: its members
//             per plane, one ballot per class and one per plane and round;
//             the lane on a session head stores the wave's counts before it
//   scan      the waves' counts per column, two levels (tiles of
//             PRIO_SCAN_TILE waves, then the tiles' sums)
//   plan      per session: per class the three totals, the counted and the
//             not-expired messages of the classes above -> the offsets that
//             turn a scanned position into C(m) and U(m); the cut class; the
//             record; popped of the classes above the cut (whole) and below
//             it (nothing)
//   classify  per message: C(m), U(m) -> disp, packet id, order, expiry_out;
//             the lane holding the Cnt-th counted message knows its member
//             index in the cut class: it writes that class's popped and what
//             the record needs of it
// No kernel waits for another workgroup, no thread loops over a session, no
// atomics on the messages.

// the heads before the wave's first message: off[r] < wbase, r < R
__device__ __forceinline__ uint32_t drain_heads_before(const DrainArgs& a, uint32_t wbase) {
    uint32_t lo = 0, hi = a.R;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.off[mid] < wbase) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint64_t drain_head_mask(const DrainArgs& a, uint64_t q0) {   // q0: the round's first message
    if (q0 >= a.Q) return 0ull;
    const uint64_t i = (q0 >> 6) * 2;
    return (uint64_t)a.heads[i] | (uint64_t)a.heads[i + 1] << 32;
}
// the scanned count of column col before wave gw (after the scan)
__device__ __forceinline__ uint32_t drain_scanned(const DrainArgs& a, uint32_t gw, uint32_t col) {
    return a.cw[(uint64_t)gw * DRAIN_COLS + col] + a.cbs[(uint64_t)(gw / PRIO_SCAN_TILE) * DRAIN_COLS + col];
}
// emqx_message:elapsed/1 (src/emqx_message.erl:296-297): max(0, Now - Since), exact for any two int64
__device__ __forceinline__ uint64_t drain_elapsed(int64_t now, int64_t since) {
    return since >= now ? 0ull : (uint64_t)now - (uint64_t)since;
}
__device__ __forceinline__ uint32_t drain_cnt(uint32_t inflight_free) {   // batch_n/1 (src/emqx_session.erl:680-684)
    return inflight_free == 0xFFFFFFFFu ? DRAIN_BATCH_N : inflight_free;
}
// the plane of a kind byte: 0 counted, 1 QoS 0 and not expired, 2 expired
__device__ __forceinline__ uint32_t drain_plane(uint32_t kind) {
    return (kind & DRAIN_EXPIRED) ? 2u : ((kind & 3u) == 0u ? 1u : 0u);
}

__global__ __launch_bounds__(256) void tm_drain_heads(DrainArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const uint32_t o = a.off[r];
    if (o < a.Q) atomicOr(a.heads + (o >> 5), 1u << (o & 31u));
    else atomicAdd(a.bad, 1u);
}

__global__ __launch_bounds__(INBOX_BLOCK) void tm_drain_count(DrainArgs a) {
    const uint32_t lane = threadIdx.x & 63, gw = blockIdx.x * (INBOX_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t wbase = (uint64_t)gw * INBOX_WAVE_PAIRS;
    if (gw >= a.nwaves) return;
    uint32_t crun[DRAIN_COLS] = {};
    if (wbase < a.Q) {
        uint32_t hb = drain_heads_before(a, (uint32_t)wbase), bad = 0;
#pragma unroll 1
        for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
            const uint64_t q = wbase + r * 64 + lane;
            const bool on = q < a.Q;
            const uint64_t hm = drain_head_mask(a, wbase + r * 64);
            const bool head = (hm >> lane) & 1ull;
            const uint32_t ri = hb + inbox_mbcnt(hm) + (head ? 1u : 0u) - 1u;   // heads at or before me, less one
            hb += (uint32_t)__popcll(hm);
            const bool ok = on && ri < a.R;
            if (on && !ok) ++bad;
            uint32_t k = on ? a.qmsg[q] : 0u;
            // is_expired/1 (src/emqx_message.erl:224-228); the product in 64 bits
            if (on && (k & DRAIN_EXPIRY) && a.created && a.expiry &&
                drain_elapsed(a.now_ms, a.created[q]) > (uint64_t)a.expiry[q] * 1000ull)
                k |= DRAIN_EXPIRED;
            if (on) a.kind[q] = (uint8_t)k;
            const uint32_t plane = drain_plane(k), cls = (k >> 4) & 7u;
            uint64_t pm[DRAIN_PLANES];
#pragma unroll
            for (uint32_t p = 0; p < DRAIN_PLANES; ++p) pm[p] = __ballot(ok && plane == p);
            uint32_t hv[DRAIN_COLS];
#pragma unroll
            for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
                const uint64_t m = c < a.ncls ? __ballot(cls == c) : 0ull;   // (wave-uniform)
#pragma unroll
                for (uint32_t p = 0; p < DRAIN_PLANES; ++p) {
                    const uint32_t col = p * PRIO_CLASSES + c;
                    hv[col] = crun[col] + inbox_mbcnt(m & pm[p]);
                    crun[col] += (uint32_t)__popcll(m & pm[p]);
                }
            }
            if (ok && head) {
                uint4* hbp = reinterpret_cast<uint4*>(a.chbase + (uint64_t)ri * DRAIN_COLS);
#pragma unroll
                for (uint32_t j = 0; j < DRAIN_COLS / 4; ++j)
                    hbp[j] = make_uint4(hv[4 * j], hv[4 * j + 1], hv[4 * j + 2], hv[4 * j + 3]);
            }
        }
        if (bad) atomicAdd(a.bad, bad);
    }
    if (lane == 0) {
        uint4* wp = reinterpret_cast<uint4*>(a.cw + (uint64_t)gw * DRAIN_COLS);
#pragma unroll
        for (uint32_t j = 0; j < DRAIN_COLS / 4; ++j)
            wp[j] = make_uint4(crun[4 * j], crun[4 * j + 1], crun[4 * j + 2], crun[4 * j + 3]);
    }
}
static_assert(DRAIN_COLS % 4 == 0, "a count vector is whole uint4s");

// Level one of the count scan, as tm_winp_scan_tiles: a block owns
// PRIO_SCAN_TILE waves of one plane (blockIdx.y), thread (segment sg, class c)
// 32 of them; exclusive in place, the tile's sums to cbs.
__global__ __launch_bounds__(256) void tm_drain_scan_tiles(DrainArgs a) {
    __shared__ uint32_t seg[32][PRIO_CLASSES];
    const uint32_t c = threadIdx.x & 7u, sg = threadIdx.x >> 3, col = blockIdx.y * PRIO_CLASSES + c;
    const uint32_t w0 = blockIdx.x * PRIO_SCAN_TILE + sg * 32u;
    uint32_t sum = 0;
    for (uint32_t i = 0; i < 32u; ++i)
        if (w0 + i < a.nwaves) sum += a.cw[(uint64_t)(w0 + i) * DRAIN_COLS + col];
    seg[sg][c] = sum;
    __syncthreads();
    uint32_t run = 0;
    for (uint32_t k = 0; k < sg; ++k) run += seg[k][c];
    if (sg == 31u) a.cbs[(uint64_t)blockIdx.x * DRAIN_COLS + col] = run + sum;
    for (uint32_t i = 0; i < 32u; ++i)
        if (w0 + i < a.nwaves) {
            const uint64_t at = (uint64_t)(w0 + i) * DRAIN_COLS + col;
            const uint32_t v = a.cw[at];
            a.cw[at] = run;
            run += v;
        }
}

// Level two: the tiles' sums, exclusive in place, and the call's totals (one
// thread per column; at most 4096 tiles, as tm_winp_scan_sums).
__global__ __launch_bounds__(64) void tm_drain_scan_sums(DrainArgs a, uint32_t nblocks) {
    const uint32_t col = threadIdx.x;
    if (col >= DRAIN_COLS) return;
    uint32_t run = 0;
    for (uint32_t k = 0; k < nblocks; ++k) {
        const uint32_t v = a.cbs[(uint64_t)k * DRAIN_COLS + col];
        a.cbs[(uint64_t)k * DRAIN_COLS + col] = run;
        run += v;
    }
    a.ctot[col] = run;
}

__global__ __launch_bounds__(256) void tm_drain_plan(DrainArgs a) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.R) return;
    const uint2 s = a.sess[r];
    const uint32_t o = a.off[r], on = a.off[r + 1];
    uint4* plan = a.plan + (uint64_t)r * PRIO_CLASSES;
    uint32_t* popped = a.popped + (uint64_t)r * PRIO_CLASSES;
    if (o >= a.Q || on > a.Q || on <= o) {   // (the host sends none such) nothing of this session is popped
#pragma unroll
        for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
            plan[c] = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
            popped[c] = 0u;
        }
        a.rec[r] = make_uint4(s.x, 0u, 0u, 0u);
        if (o < a.Q) atomicAdd(a.bad, 1u);   // (tm_drain_heads counted the other case)
        return;
    }
    const uint32_t wo = o / INBOX_WAVE_PAIRS, wn = on / INBOX_WAVE_PAIRS;
    const bool last = r + 1 >= a.R;
    const uint32_t cnt = drain_cnt(s.y);
    uint32_t cumK = 0, cumU = 0, cumA = 0;   // counted / not expired / all messages of the classes above
    uint32_t z_all = 0, x_all = 0;           // QoS 0 not expired / expired messages popped with whole classes
    bool cut = cnt == 0;                     // the class holding the Cnt-th counted message is at or above c
#pragma unroll
    for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
        uint32_t base[DRAIN_PLANES], tot[DRAIN_PLANES];
#pragma unroll
        for (uint32_t p = 0; p < DRAIN_PLANES; ++p) {
            const uint32_t col = p * PRIO_CLASSES + c;
            base[p] = drain_scanned(a, wo, col) + a.chbase[(uint64_t)r * DRAIN_COLS + col];
            const uint32_t next = last ? a.ctot[col] : drain_scanned(a, wn, col) + a.chbase[(uint64_t)(r + 1) * DRAIN_COLS + col];
            tot[p] = next - base[p];
        }
        const uint32_t K = tot[0], Z = tot[1], X = tot[2];
        // behind the cut nothing is popped: C(m) >= Cnt there whatever the offsets say, so they may stay exact
        plan[c] = make_uint4(cumK - base[0], cumU - (base[0] + base[1]), base[0] + base[1] + base[2], cumA);
        const bool whole = !cut && cumK + K < cnt;   // every message of the class has C(m) < Cnt
        popped[c] = whole ? K + Z + X : 0u;          // the cut class: the lane of the Cnt-th counted message writes it
        if (whole) { z_all += Z; x_all += X; }
        else cut = true;
        cumK += K;
        cumU += K + Z;
        cumA += K + Z + X;
    }
    const uint32_t nsend = min(cumK, cnt);
    // cumK >= Cnt > 0: the lane of the Cnt-th counted message writes n_send0 and n_expired
    a.rec[r] = make_uint4((s.x - 1u + nsend % 65535u) % 65535u + 1u, nsend, z_all, x_all);
}

__global__ __launch_bounds__(INBOX_BLOCK) void tm_drain_classify(DrainArgs a) {
    const uint32_t lane = threadIdx.x & 63, gw = blockIdx.x * (INBOX_BLOCK / 64) + (threadIdx.x >> 6);
    const uint64_t wbase = (uint64_t)gw * INBOX_WAVE_PAIRS;
    if (gw >= a.nwaves) return;
    uint32_t tot[DRAIN_NDISP] = {};
    if (wbase < a.Q) {
        uint32_t crun[DRAIN_COLS];
#pragma unroll
        for (uint32_t col = 0; col < DRAIN_COLS; ++col) crun[col] = drain_scanned(a, gw, col);
        uint32_t hb = drain_heads_before(a, (uint32_t)wbase);
#pragma unroll 1
        for (uint32_t r = 0; r < INBOX_ROUNDS; ++r) {
            const uint64_t q = wbase + r * 64 + lane;
            const bool on = q < a.Q;
            const uint64_t hm = drain_head_mask(a, wbase + r * 64);
            const uint32_t ri = hb + inbox_mbcnt(hm) + (uint32_t)((hm >> lane) & 1ull) - 1u;
            hb += (uint32_t)__popcll(hm);
            const bool ok = on && ri < a.R;   // (tm_drain_count counted the others)
            const uint32_t k = on ? a.kind[q] : 0u;
            const uint32_t plane = drain_plane(k), cls = (k >> 4) & 7u;
            uint64_t pm[DRAIN_PLANES];
#pragma unroll
            for (uint32_t p = 0; p < DRAIN_PLANES; ++p) pm[p] = __ballot(ok && plane == p);
            uint32_t mine[DRAIN_PLANES] = {};   // the scanned counts of my class before me
#pragma unroll
            for (uint32_t c = 0; c < PRIO_CLASSES; ++c) {
                const uint64_t m = c < a.ncls ? __ballot(cls == c) : 0ull;   // (wave-uniform)
#pragma unroll
                for (uint32_t p = 0; p < DRAIN_PLANES; ++p) {
                    const uint32_t col = p * PRIO_CLASSES + c;
                    if (cls == c) mine[p] = crun[col] + inbox_mbcnt(m & pm[p]);
                    crun[col] += (uint32_t)__popcll(m & pm[p]);
                }
            }
            const uint2 s = ok ? a.sess[ri] : make_uint2(1u, 0u);
            const uint4 pl = ok ? a.plan[(uint64_t)ri * PRIO_CLASSES + cls] : make_uint4(0u, 0u, 0u, 0u);
            const uint32_t cnt = drain_cnt(s.y);
            const uint32_t C = mine[0] + pl.x, U = mine[0] + mine[1] + pl.y;
            const uint32_t member = mine[0] + mine[1] + mine[2] - pl.z;   // my index among my class's messages
            const bool pop = ok && C < cnt;
            uint32_t d = 2u, id = 0u, ord = 0xFFFFFFFFu;                        // TM_DRAIN_KEPT
            if (pop) {
                if (plane == 2u) d = 3u;                                        // TM_DRAIN_EXPIRED
                else {
                    ord = U;
                    if (plane == 1u) d = 0u;                                    // TM_DRAIN_SEND0
                    else { d = 1u; id = (s.x - 1u + C % 65535u) % 65535u + 1u; }   // TM_DRAIN_SEND
                }
            }
            if (on) {
                a.disp[q] = (uint8_t)d;
                a.pid[q] = (uint16_t)id;
                a.order[q] = ord;
                if (a.expiry_out) {
                    uint32_t e = a.expiry ? a.expiry[q] : 0u;
                    if (d < 2u && (k & DRAIN_EXPIRY) && a.created && a.expiry) {   // update_expiry/1 (src/emqx_message.erl:230-239)
                        const uint64_t el = drain_elapsed(a.now_ms, a.created[q]);
                        if (el > 0) e = (uint32_t)max<uint64_t>(1ull, (uint64_t)e - min<uint64_t>(el / 1000ull, e));
                    }
                    a.expiry_out[q] = e;
                }
            }
            if (pop && plane == 0u && C + 1u == cnt) {   // the Cnt-th counted message: dequeue/3 stops behind it
                a.popped[(uint64_t)ri * PRIO_CLASSES + cls] = member + 1u;
                uint32_t* rec = reinterpret_cast<uint32_t*>(a.rec + ri);
                rec[2] = U + 1u - cnt;                       // not expired and popped, less the counted ones
                rec[3] = pl.w + member + 1u - (U + 1u);      // popped, less the not expired ones
            }
#pragma unroll
            for (uint32_t j = 0; j < DRAIN_NDISP; ++j) tot[j] += (uint32_t)__popcll(__ballot(on && d == j));
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t j = 0; j < DRAIN_NDISP; ++j) a.wdisp[(uint64_t)gw * DRAIN_NDISP + j] = tot[j];
    }
}

// the waves' disposition counts -> totals (one block), as tm_window_totals
__global__ __launch_bounds__(256) void tm_drain_totals(DrainArgs a) {
    __shared__ unsigned long long sh[4][DRAIN_NDISP];
    unsigned long long v[DRAIN_NDISP] = {};
    for (uint32_t i = threadIdx.x; i < a.nwaves; i += 256)
#pragma unroll
        for (uint32_t k = 0; k < DRAIN_NDISP; ++k) v[k] += a.wdisp[(uint64_t)i * DRAIN_NDISP + k];
#pragma unroll
    for (uint32_t k = 0; k < DRAIN_NDISP; ++k) {
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < DRAIN_NDISP) {
        const uint32_t k = threadIdx.x;
        a.totals[k] = sh[0][k] + sh[1][k] + sh[2][k] + sh[3][k];
    }
}

// The global table: a slot holds ONE topic, {1 | 10 hash bits | length (13
// bits) | byte offset (40 bits)}.  A claim probes from the hash's home; an
// occupant with the same hash bits and length has its bytes compared, and
// only equal bytes join it (lowering the offset with atomicMin: the topic's
// first occurrence has the lowest offset -- offsets grow with the publish
// index, strictly for non-empty topics); anything else probes on.  So a
// slot's topic never changes once claimed, and a hash collision costs a
// probe, never a wrong row.
constexpr uint64_t DD_OFF_MASK = (1ull << DD_OFF_BITS) - 1ull;

// Slots are read with PLAIN loads (this XCD's L2, not the device-coherent
// path): a stale copy can only be 0 (then the CAS returns the slot's value)
// or an older offset of the slot's own topic (equal bytes all the same) --
// a slot's topic never changes.
__device__ __forceinline__ unsigned long long dd_want(uint64_t h, uint64_t b, uint32_t len) {
    return (1ull << 63) | (((h >> 54) & 0x3FFull) << 53) | ((uint64_t)len << DD_OFF_BITS) | b;
}

__device__ __forceinline__ uint32_t dd_claim(const DedupArgs& a, uint64_t h, uint64_t b, uint32_t len,
                                             const uint32_t (&c)[16]) {
    const unsigned long long want = dd_want(h, b, len);
    uint64_t i = h & a.mask;
    for (;;) {
        unsigned long long v = a.table[i];
        if (v == 0) {
            v = atomicCAS(&a.table[i], 0ull, want);
            if (v == 0) return (uint32_t)i;
        }
        if ((v >> DD_OFF_BITS) == (want >> DD_OFF_BITS) && dd_equal(a.bytes, c, b, v & DD_OFF_MASK, len)) {
            if (b < (v & DD_OFF_MASK)) atomicMin(&a.table[i], want);
            return (uint32_t)i;
        }
        i = (i + 1) & a.mask;
    }
}

// Pass 1 (claim), one thread per publish, its bytes in registers.  A
// publish whose topic already holds its home slot joins it at once.  C5's
// hot topics would put hundreds of thousands of claims on one slot's line
// (Zipf over 10k hot topics, the first ~9% of the publishes), so the others
// first collapse in the workgroup's LDS: equal hashes elect the lowest thread,
// whose bytes each follower compares with its own (a follower whose bytes
// differ -- a 64-bit collision -- takes part in the next round's election), and
// only the leaders claim global slots; followers take their leader's.
constexpr uint32_t DD_BLOCK = 256;
constexpr uint32_t DD_LT = 512;       // LDS election slots (load <= 1/2)

__global__ __launch_bounds__(DD_BLOCK) void tm_dedup_claim(DedupArgs a) {
    __shared__ unsigned long long lkey[DD_LT];
    __shared__ uint32_t lmin[DD_LT];
    __shared__ uint32_t lslot[DD_BLOCK];
    __shared__ uint64_t lb[DD_BLOCK];
    __shared__ uint32_t ll[DD_BLOCK];
    __shared__ uint32_t lc[16][DD_BLOCK];   // every publish's first 64 bytes: a follower checks its leader's here
    const uint32_t tid = threadIdx.x;
    const uint32_t t = blockIdx.x * DD_BLOCK + tid;
    const bool valid = t < a.n;
    uint64_t b = 0, h = 0;
    uint32_t len = 0;
    if (valid) {
        b = a.offs[t] - a.base;
        len = (uint32_t)(a.offs[t + 1] - a.base - b);
    }
    bool resolved = false;
    uint32_t rslot = 0;
    {
        uint32_t c[16];
        dd_load64(a.bytes, b, len, c);
        if (valid) {
            h = dd_hash(a.bytes, b, len, c);
            if (a.weak_hash) h = ((uint64_t)len << 40) | ((uint64_t)len << 8) | 1ull;
            // a topic already in its home slot (the common case once a hot
            // topic has been claimed: C5's 90% hot publishes) joins it here,
            // two L2 reads, no election and no atomic
            const uint64_t i = h & a.mask;
            const unsigned long long want = dd_want(h, b, len), v = a.table[i];
            if (v && (v >> DD_OFF_BITS) == (want >> DD_OFF_BITS) && dd_equal(a.bytes, c, b, v & DD_OFF_MASK, len)) {
                if (b < (v & DD_OFF_MASK)) atomicMin(&a.table[i], want);
                resolved = true;
                rslot = (uint32_t)i;
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 16; ++q) lc[q][tid] = c[q];
    }
    lb[tid] = b;
    ll[tid] = len;
    bool pend = valid && !resolved, leader = false;
    uint32_t lead = tid, s = 0;
    while (__syncthreads_or(pend)) {
        for (uint32_t k = tid; k < DD_LT; k += DD_BLOCK) {
            lkey[k] = 0;
            lmin[k] = NONE;
        }
        __syncthreads();
        if (pend) {
            s = (uint32_t)(h >> 7) & (DD_LT - 1);
            for (;;) {
                const unsigned long long o = atomicCAS(&lkey[s], 0ull, (unsigned long long)(h | 1ull));
                if (o == 0 || o == (h | 1ull)) break;
                s = (s + 1) & (DD_LT - 1);
            }
            atomicMin(&lmin[s], tid);
        }
        __syncthreads();
        if (pend) {
            const uint32_t L = lmin[s];
            if (L == tid) {
                leader = true;
                pend = false;
            } else if (ll[L] == len) {   // the leader's first 64 bytes from LDS, the rest (long topics) from HBM
                uint32_t diff = 0;
#pragma unroll
                for (uint32_t q = 0; q < 16; ++q) diff |= lc[q][L] ^ lc[q][tid];
                bool eq = diff == 0;
                if (eq && len > 64u) {
                    uint32_t c[16];
#pragma unroll
                    for (uint32_t q = 0; q < 16; ++q) c[q] = lc[q][tid];
                    eq = dd_equal(a.bytes, c, b, lb[L], len);
                }
                if (eq) {
                    lead = L;
                    pend = false;
                }
            }
        }
    }
    if (leader) {
        uint32_t c[16];
#pragma unroll
        for (uint32_t q = 0; q < 16; ++q) c[q] = lc[q][tid];
        lslot[tid] = dd_claim(a, h, b, len, c);
    }
    __syncthreads();
    if (valid) a.slot[t] = resolved ? rslot : lslot[lead];
}

// Pass 2 (count): publish t is its topic's representative when its offset is
// the slot's (an empty topic: the first of the empty publishes at that
// offset).  Ballots -> repbits; per DD_TILE block the representatives and
// their bytes -> bcount / bbytes (scanned next).  4 independent slot ->
// table chains per thread in flight (DD_PT publishes, 256 apart).
constexpr uint32_t DD_PT = DD_TILE / 256;

__global__ __launch_bounds__(256) void tm_dedup_count(DedupArgs a) {
    __shared__ uint32_t sc[4], sb[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t t0 = blockIdx.x * DD_TILE;
    // every load of a stage issued before the next stage's: slot + offsets,
    // then the table (4 independent chains per thread)
    uint32_t sl[DD_PT];
    uint64_t o0[DD_PT], o1[DD_PT];
#pragma unroll
    for (uint32_t u = 0; u < DD_PT; ++u) {
        const uint32_t t = t0 + u * 256 + tid;
        const bool in = t < a.n;
        sl[u] = in ? a.slot[t] : 0u;
        o0[u] = in ? a.offs[t] : 0ull;
        o1[u] = in ? a.offs[t + 1] : 0ull;
    }
    unsigned long long v[DD_PT];
#pragma unroll
    for (uint32_t u = 0; u < DD_PT; ++u) v[u] = (t0 + u * 256 + tid < a.n) ? a.table[sl[u]] : 0ull;
    uint32_t cnt = 0, byt = 0;
#pragma unroll
    for (uint32_t u = 0; u < DD_PT; ++u) {
        const uint32_t t = t0 + u * 256 + tid;
        const uint32_t len = (uint32_t)(o1[u] - o0[u]);
        bool rep = t < a.n && (v[u] & DD_OFF_MASK) == o0[u] - a.base;
        if (rep && !len && t) rep = a.offs[t - 1] != o0[u];   // (empty topics: the first at that offset)
        const uint64_t bits = __ballot(rep);
        if ((tid & 63) == 0) a.repbits[(t0 + u * 256 + tid) / 64] = bits;
        cnt += rep ? 1u : 0u;
        byt += rep ? len : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o, 64);
        byt += __shfl_xor(byt, o, 64);
    }
    if ((tid & 63) == 0) {
        sc[tid >> 6] = cnt;
        sb[tid >> 6] = byt;
    }
    __syncthreads();
    if (tid == 0) {
        a.bcount[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
        a.bbytes[blockIdx.x] = sb[0] + sb[1] + sb[2] + sb[3];
    }
}

// exclusive scan of one u64 per thread over a 256-thread block (-> the block total)
__device__ __forceinline__ uint64_t block256_excl_scan(uint64_t v, uint64_t* sh, uint64_t& total) {
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t incl = v;
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up(incl, o, 64);
        if (lane >= o) incl += u;
    }
    if (lane == 63) sh[wid] = incl;
    __syncthreads();
    uint64_t base = 0;
    for (uint32_t w = 0; w < wid; ++w) base += sh[w];
    total = sh[0] + sh[1] + sh[2] + sh[3];
    return base + incl - v;
}

// Pass 3 (compact), same blocks, 4 consecutive publishes per thread (DD_PT): every
// representative's row and byte offset (block base from the scans + its rank
// in the block), its bytes copied into the tokeniser's input, and
// srow[slot] = row, rrep[row] = publish for the expansion.  A thread's
// representatives get consecutive rows and one contiguous byte range, which it
// writes as aligned dwords assembled in a shift register (byte stores only
// for the partial dwords at its two ends, shared with its neighbours): the
// first blocks hold most first occurrences (C5: ~1,900 of the first 4,096
// publishes), and byte stores made them the kernel's tail; 4 publishes per
// thread keep a thread's serial representatives few.
__device__ __forceinline__ void dd_put(uint8_t* dst, uint64_t lo, uint64_t hi, uint64_t& acc, uint32_t& bits,
                                       uint64_t& w, uint32_t v, uint32_t nb) {
    // append nb (<= 4) bytes of v at dword w's bit `bits`; full dwords inside
    // [lo, hi) are stored whole, a dword reaching outside byte by byte
    acc |= (uint64_t)v << bits;
    bits += 8u * nb;
    if (bits >= 32u) {
        const uint64_t d0 = w * 4;
        if (d0 >= lo && d0 + 4 <= hi) {
            *reinterpret_cast<uint32_t*>(dst + d0) = (uint32_t)acc;
        } else {
            for (uint32_t q = 0; q < 4; ++q)
                if (d0 + q >= lo && d0 + q < hi) dst[d0 + q] = (uint8_t)(acc >> (8 * q));
        }
        acc >>= 32;
        bits -= 32u;
        ++w;
    }
}

__global__ __launch_bounds__(256) void tm_dedup_compact(DedupArgs a) {
    __shared__ uint64_t sh[4];
    const uint32_t tid = threadIdx.x;
    const uint32_t nblk = dedup_blocks(a.n);
    const uint32_t first = blockIdx.x * DD_TILE + tid * DD_PT;
    const uint32_t row0 = a.bcount[blockIdx.x] + a.rbs[blockIdx.x / SCAN_TILE];
    const uint64_t off0 = (uint64_t)a.bbytes[blockIdx.x] + a.bbs[blockIdx.x / SCAN_TILE];
    const uint32_t mine = (uint32_t)(a.repbits[first / 64] >> (first & 63)) & ((1u << DD_PT) - 1u);
    uint32_t my_bytes = 0;
#pragma unroll
    for (uint32_t j = 0; j < DD_PT; ++j) {
        if ((mine >> j) & 1u) {
            const uint32_t t = first + j;
            my_bytes += (uint32_t)(a.offs[t + 1] - a.offs[t]);
        }
    }
    uint64_t tot;
    const uint64_t ex = block256_excl_scan(((uint64_t)my_bytes << 16) | (uint64_t)__popc(mine), sh, tot);
    uint32_t row = row0 + (uint32_t)(ex & 0xFFFFu);
    const uint64_t lo = off0 + (ex >> 16), hi = lo + my_bytes;   // this thread's bytes in cbytes
    uint64_t off = lo;
    if (blockIdx.x == 0 && tid == 0) {   // totals: the scans left them at [nblk]
        a.dd[0] = a.bcount[nblk];
        a.coffs[a.bcount[nblk]] = a.bbytes[nblk];
    }
    uint64_t acc = 0, w = lo >> 2;
    uint32_t bits = 8u * (uint32_t)(lo & 3u);
    for (uint32_t rest = mine; rest; rest &= rest - 1) {   // (representatives are few: not unrolled)
        const uint32_t t = first + (uint32_t)__ffs(rest) - 1u;
        a.srow[a.slot[t]] = row;
        a.rrep[row] = t;
        a.coffs[row] = off;
        const uint64_t b = a.offs[t] - a.base;
        const uint32_t n = (uint32_t)(a.offs[t + 1] - a.offs[t]);
        for (uint32_t k = 0; k < n; k += 64) {
            uint32_t x[16];
            dd_load64(a.bytes, b + k, n - k, x);
            const uint32_t m = n - k < 64u ? n - k : 64u;
#pragma unroll
            for (uint32_t q = 0; q < 16; ++q) {
                if (4u * q >= m) break;
                const uint32_t nb = m - 4u * q < 4u ? m - 4u * q : 4u;
                dd_put(a.cbytes, lo, hi, acc, bits, w, x[q], nb);   // (x is zero past the topic)
            }
        }
        ++row;
        off += n;
    }
    if (bits && hi > lo) {   // the last partial dword
        const uint64_t d0 = w * 4;
        for (uint32_t q = 0; q < 4; ++q)
            if (d0 + q >= lo && d0 + q < hi) a.cbytes[d0 + q] = (uint8_t)(acc >> (8 * q));
    }
}

// After the walk, per row (a grid-stride loop over the device-counted rows):
// its (count, start) go to smeta at its table slot, and the slot is cleared
// (nothing reads the table after the compaction): the next dedup pass finds it
// zero without a memset.
__global__ __launch_bounds__(256) void tm_dedup_rowmeta(DedupArgs a) {
    const uint32_t rows = *a.dd;
    for (uint32_t r = blockIdx.x * 256 + threadIdx.x; r < rows; r += gridDim.x * 256) {
        const uint32_t s = a.slot[a.rrep[r]];
        const unsigned long long sr = a.src[r];
        a.smeta[s] = uint4{a.count[r], 0u, (uint32_t)sr, (uint32_t)(sr >> 32)};
        a.table[s] = 0;
    }
}

// Then every publish gets its row's (count, start) -- the result per publish
// -- through its slot: slot[t], then smeta[slot] (the hot topics' entries
// stay in L2), and the batch's delivered matches are summed per block.
constexpr uint32_t EXPAND_PER_THREAD = DD_EXPAND_TILE / 256;
__global__ __launch_bounds__(256) void tm_dedup_expand(DedupArgs a) {
    __shared__ unsigned long long sh[4];
    const uint32_t base = blockIdx.x * 256 * EXPAND_PER_THREAD + threadIdx.x;
    // staged: every slot, then every slot's (count, start) -- each stage's
    // loads in flight together
    uint32_t sl[EXPAND_PER_THREAD];
#pragma unroll
    for (uint32_t u = 0; u < EXPAND_PER_THREAD; ++u) {
        const uint32_t t = base + u * 256;
        sl[u] = t < a.n ? a.slot[t] : 0u;
    }
    uint4 m[EXPAND_PER_THREAD];
#pragma unroll
    for (uint32_t u = 0; u < EXPAND_PER_THREAD; ++u) m[u] = base + u * 256 < a.n ? a.smeta[sl[u]] : uint4{0u, 0u, 0u, 0u};
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t u = 0; u < EXPAND_PER_THREAD; ++u) {
        const uint32_t t = base + u * 256;
        if (t < a.n) {
            a.pcount[t] = m[u].x;
            a.psrc[t] = ((unsigned long long)m[u].w << 32) | m[u].z;
            sum += m[u].x;
        }
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = sum;
    __syncthreads();
    // a partial sum per block, added up by tm_dedup_sum: one same-address
    // atomic per block serialised at ~30 ns each (4,883 blocks: ~0.15 ms)
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// row_of[t] = srow[slot[t]]: the publish -> row map, built only when the host
// asks for it (tm_batch_row_map) -- the per-launch expansion skips the 40 MB
__global__ __launch_bounds__(256) void tm_dedup_rowof(DedupArgs a) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t < a.n) a.row_of[t] = a.srow[a.slot[t]];
}

// the expansion's block sums -> the batch's delivered matches; the rows for
// the host's read-back
__global__ __launch_bounds__(1024) void tm_dedup_sum(DedupArgs a, uint32_t nb) {
    __shared__ unsigned long long sh[16];
    unsigned long long s = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += 1024) s += a.bsum[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < 16; ++w) t += sh[w];
        if (t) atomicAdd(&a.stats[ST_DELIVERED], t);
        a.ctrl[CTRL_NROWS] = a.dd[0];
    }
}

// ------------------------------------------------ sampled rows (tm_batch_sample)

// A few rows of a waited batch, as the walk left them (count + start into the
// staging area), gathered into a compact CSR: the multi-device self-check
// reads ~3,000 rows per slice this way instead of a whole 10M-row CSR.
__global__ __launch_bounds__(256) void tm_sample_meta(const uint32_t* count, const unsigned long long* src,
                                                       const uint32_t* rows, uint32_t k, uint32_t* out_cnt,
                                                       unsigned long long* out_src) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const uint32_t r = rows[i];
    out_cnt[i] = count[r];
    out_src[i] = src[r];
}

// one wave per sampled row: its ids to out[off[i] ..)
__global__ __launch_bounds__(64) void tm_sample_ids(const uint32_t* sfids, const uint32_t* cnt,
                                                     const unsigned long long* src, const uint64_t* off,
                                                     uint32_t* out) {
    const uint32_t i = blockIdx.x;
    const uint32_t c = cnt[i];
    const unsigned long long s = src[i];
    const uint64_t o = off[i];
    for (uint32_t j = threadIdx.x; j < c; j += 64) out[o + j] = sfids[s + j];
}

// ------------------------------------------------ token batches (sharded mode)

// Row gather for the sharded exchange: 16 lanes per row (rows are short: the
// words of a topic, or one topic's match list), lanes stride over long rows.
__global__ __launch_bounds__(256) void tm_gather_rows(const uint32_t* src, const int64_t* src_off, const int64_t* idx,
                                                       uint32_t n, const int64_t* dst_off, uint32_t* dst) {
    const uint64_t g = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15;
    if (g >= n) return;
    const int64_t r = idx[g];
    const int64_t b = src_off[r], e = src_off[r + 1], d = dst_off[g];
    for (int64_t i = sub; i < e - b; i += 16) dst[d + i] = src[b + i];
}

// Validates a device-resident token batch before any walk reads it (toff
// monotone from 0 to nwords, deep topics flagged for the generic path) and
// compacts the generic-path topics into slow_list / *d_nslow.  Any violation
// sets *d_bad; the host refuses the batch.
__global__ __launch_bounds__(256) void tm_token_check(const uint32_t* toff, const uint8_t* tflags, uint32_t n,
                                                       uint64_t nwords, uint32_t* slow_list, uint32_t* d_nslow,
                                                       uint32_t* d_bad) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63;
    bool slow = false;
    if (t < n) {
        const uint32_t b = toff[t], e = toff[t + 1];
        const uint8_t f = tflags[t];
        const bool ok = b <= e && (uint64_t)e <= nwords && (t > 0 || b == 0) && (t + 1 < n || (uint64_t)e == nwords) &&
                        (f & ~(TF_DOLLAR | TF_SLOW)) == 0 && (e - b <= FAST_MAX_DEPTH || (f & TF_SLOW));
        if (!ok) atomicOr(d_bad, 1u);
        slow = ok && (f & TF_SLOW);
    }
    const uint64_t m = __ballot(slow);
    if (!m) return;
    const uint32_t first = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == first) base = atomicAdd(d_nslow, (uint32_t)__popcll(m));
    base = __shfl(base, first, 64);
    if (slow) slow_list[base + prefix_count(m)] = t;
}

// Shard of each topic (tm_filter_shard's rule on the topic side): the shard of
// its first two words when both are interned literals, else nshards (every
// shard resolves it: only replicated filters can match).
__global__ __launch_bounds__(256) void tm_tokens_shard(const uint32_t* words, const uint32_t* toff, uint32_t n,
                                                        uint32_t nshards, uint32_t* shard) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const uint32_t b = toff[t], d = toff[t + 1] - b;
    uint32_t s = nshards;
    if (d >= 2) {
        const uint32_t i0 = words[b] & WID_MASK, i1 = words[b + 1] & WID_MASK;
        const bool lit0 = i0 != W_UNKNOWN && i0 != W_PLUS && i0 != W_HASH;
        const bool lit1 = i1 != W_UNKNOWN && i1 != W_PLUS && i1 != W_HASH;
        if (lit0 && lit1) s = prefix_shard(i0, i1, nshards);
    }
    shard[t] = s;
}

// ---------------------------------------- in-process filter-sharded group

// The publish's owner: its shard, or (G = any shard resolves it: only
// replicated filters can match) spread round-robin by publish index.
__device__ __forceinline__ uint32_t part_owner(const PartArgs& a, uint32_t t) {
    const uint32_t o = a.owner[t];
    return o < a.G ? o : t % a.G;
}

__device__ __forceinline__ uint32_t scan_at(const uint32_t* off, const uint32_t* bs, uint32_t i) {
    return off[i] + bs[i / SCAN_TILE];
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Pass 1: per block and owner, publishes and words -> cnt / wcnt (g-major, so
// one scan over them numbers each owner's publishes contiguously).
__global__ __launch_bounds__(PART_BLOCK) void tm_part_count(PartArgs a) {
    __shared__ uint32_t sc[PART_BLOCK / 64][PART_MAX_G], sw[PART_BLOCK / 64][PART_MAX_G];
    const uint32_t t = blockIdx.x * PART_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const bool valid = t < a.n;
    const uint32_t g_me = valid ? part_owner(a, t) : a.G;
    const uint32_t depth = valid ? a.toff[t + 1] - a.toff[t] : 0u;
    for (uint32_t g = 0; g < a.G; ++g) {
        const uint64_t m = __ballot(g_me == g);
        const uint32_t w = wave_sum(g_me == g ? depth : 0u);
        if (lane == 0) { sc[wid][g] = (uint32_t)__popcll(m); sw[wid][g] = w; }
    }
    __syncthreads();
    for (uint32_t g = threadIdx.x; g < a.G; g += PART_BLOCK) {
        uint32_t c = 0, w = 0;
        for (uint32_t k = 0; k < PART_BLOCK / 64; ++k) { c += sc[k][g]; w += sw[k][g]; }
        a.cnt[g * a.nb + blockIdx.x] = c;
        a.wcnt[g * a.nb + blockIdx.x] = w;
    }
}

// segs[g] = first partitioned position of owner g (segs[G] = n), segs[G + 1 + g]
// = its first word (segs[2G + 1] = all words): the host sizes each shard's part.
__global__ void tm_part_segs(PartArgs a) {
    const uint32_t g = threadIdx.x;
    if (g > a.G) return;
    const uint32_t i = g * a.nb;
    a.segs[g] = g < a.G ? scan_at(a.cnt_off, a.cnt_bs, i) : a.cnt_off[a.G * a.nb];
    a.segs[a.G + 1 + g] = g < a.G ? scan_at(a.w_off, a.w_bs, i) : a.w_off[a.G * a.nb];
}

// Pass 3: every publish to its place in its owner's part, with its words; the
// part's word offsets restart at wbase[g] (where the part lands in owner g's
// token batch, after the parts of earlier slices), so part g's offsets sit at
// ptoff[segs[g] + g ..] ready to be copied.
__global__ __launch_bounds__(PART_BLOCK) void tm_part_scatter(PartArgs a) {
    __shared__ uint32_t sc[PART_BLOCK / 64][PART_MAX_G], sw[PART_BLOCK / 64][PART_MAX_G];
    const uint32_t t = blockIdx.x * PART_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const bool valid = t < a.n;
    const uint32_t g_me = valid ? part_owner(a, t) : a.G;
    const uint32_t depth = valid ? a.toff[t + 1] - a.toff[t] : 0u;
    uint32_t rank = 0, wpre = 0;
    for (uint32_t g = 0; g < a.G; ++g) {
        const bool mine = g_me == g;
        const uint64_t m = __ballot(mine);
        // inclusive scan of this owner's depths across the wave
        uint32_t incl = mine ? depth : 0u;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += u;
        }
        if (mine) { rank = prefix_count(m); wpre = incl - depth; }
        if (lane == 63) { sc[wid][g] = (uint32_t)__popcll(m); sw[wid][g] = incl; }
    }
    __syncthreads();
    // each part's closing offset (its word count)
    if (blockIdx.x == 0 && threadIdx.x < a.G) {
        const uint32_t g = threadIdx.x;
        const uint32_t tend = g + 1 < a.G ? scan_at(a.cnt_off, a.cnt_bs, (g + 1) * a.nb) : a.cnt_off[a.G * a.nb];
        const uint32_t wend = g + 1 < a.G ? scan_at(a.w_off, a.w_bs, (g + 1) * a.nb) : a.w_off[a.G * a.nb];
        a.ptoff[tend + g] = wend - scan_at(a.w_off, a.w_bs, g * a.nb) + a.wbase[g];
    }
    if (!valid) return;
    uint32_t bt = 0, bw = 0;   // earlier waves of the block, same owner
    for (uint32_t k = 0; k < wid; ++k) { bt += sc[k][g_me]; bw += sw[k][g_me]; }
    const uint32_t i = g_me * a.nb + blockIdx.x;
    const uint32_t p = scan_at(a.cnt_off, a.cnt_bs, i) + bt + rank;
    const uint32_t w = scan_at(a.w_off, a.w_bs, i) + bw + wpre;
    const uint32_t wseg = scan_at(a.w_off, a.w_bs, g_me * a.nb);
    a.order[p] = t + a.tbase;
    const uint32_t src = a.toff[t];
    const uint32_t woff = w - wseg + a.wbase[g_me];   // in owner g's batch
    if (a.dtoff[g_me]) {   // straight into the owner's batch (local, or a peer's HBM)
        const uint32_t tseg = scan_at(a.cnt_off, a.cnt_bs, g_me * a.nb);
        const uint32_t q = p - tseg + a.rbase[g_me];
        a.dflags[g_me][q] = a.tflags[t];
        a.dtoff[g_me][q] = woff;
        uint32_t* dw = a.dwords[g_me] + woff;
        for (uint32_t k = 0; k < depth; ++k) dw[k] = a.words[src + k];
        return;
    }
    a.ptflags[p] = a.tflags[t];
    a.ptoff[p + g_me] = woff;
    for (uint32_t k = 0; k < depth; ++k) a.pwords[w + k] = a.words[src + k];
}

__global__ __launch_bounds__(256) void tm_unpart_counts(const uint32_t* order, const uint32_t* counts_p, uint32_t n,
                                                         uint32_t* counts_o) {
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) counts_o[order[p]] = counts_p[p];
}

// 16 lanes per row (rows are short lists of filter ids; lanes stride long ones)
__global__ __launch_bounds__(256) void tm_unpart_rows(const uint32_t* order, const uint32_t* counts_p, uint32_t n,
                                                       const uint32_t* src_off, const uint32_t* src_bs,
                                                       const uint32_t* dst_off, const uint32_t* dst_bs,
                                                       const uint32_t* ids_p, uint32_t* out, uint32_t* rowg) {
    const uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15;
    if (p > n) return;
    if (p == n) {   // the closing offset
        if (sub == 0) rowg[n] = dst_off[n];
        return;
    }
    const uint32_t t = order[p];
    const uint32_t len = counts_p[p];
    const uint32_t src = scan_at(src_off, src_bs, (uint32_t)p), dst = scan_at(dst_off, dst_bs, t);
    if (sub == 0) rowg[t] = dst;
    for (uint32_t k = sub; k < len; k += 16) out[dst + k] = ids_p[src + k];
}

// counts[t] = |row t|; gids[i] = ids[i] * mul + add (a shard's global ids).
__global__ __launch_bounds__(256) void tm_export(const uint32_t* row_off, const uint32_t* ids, uint32_t n, uint64_t total,
                                                  uint32_t* counts, uint32_t* gids, uint32_t mul, uint32_t add) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) gids[i] = ids[i] * mul + add;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) counts[i] = row_off[i + 1] - row_off[i];
}

__global__ void tm_scatter_slots(Slot* slots, const uint32_t* idx, const Slot* vals, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) slots[idx[i]] = vals[i];
}

__global__ void tm_scatter_fmeta(uint64_t* foff, uint32_t* flen, const uint32_t* idx, const uint64_t* off,
                                 const uint32_t* len, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { foff[idx[i]] = off[i]; flen[idx[i]] = len[i]; }
}

// ------------------------------------------------------------ device tokeniser
// emqx_topic:words/1 (src/emqx_topic.erl:150-164: binary:split on "/", '' / '+'
// / '#' as their atoms) plus the engine's interning, on the device: the same
// word entries (class << 29 | id), flags and generic-path list as the host
// tokeniser (tm_batch.cpp tokenize_range).  One wavefront per tile of 64
// topics, whose bytes are contiguous in the batch:
//   tm_tok_count  words per tile = '/' bytes in the tile's range + topics,
//                 counted from coalesced dword loads (bit tricks, no per-byte
//                 loop); also clears the launch's control words;
//   (scan of the tile counts)
//   tm_tok_fill   the tile's bytes are staged in LDS by coalesced loads; each
//                 lane splits its own topic there (word starts / lengths into
//                 an LDS list, flags, in-tile word offsets by a wave scan);
//                 then the lanes take the tile's WORDS round-robin -- class,
//                 reserved atoms, dictionary probe with the first 8 bytes
//                 compared inline -- and the tile's words leave LDS as one
//                 coalesced run.  Tiles too long for the LDS budget take a
//                 lane-per-topic path that reads the bytes from HBM.

constexpr uint32_t TOK_LANE_BYTES = 48;                 // bytes of the window each lane splits
constexpr uint32_t TOK_BYTES = 64 * TOK_LANE_BYTES;     // LDS bytes per tile (16-B aligned window)
constexpr uint32_t TOK_WORDS = 512;                     // words per tile on the LDS path

// bytes with value v in the 4 bytes of x (SWAR): each matching byte -> 0x80
__device__ __forceinline__ uint32_t byte_eq(uint32_t x, uint32_t v) {
    const uint32_t y = x ^ (v * 0x01010101u);
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y | 0x7F7F7F7Fu);
}

__device__ __forceinline__ uint32_t tok_class(uint8_t c0, uint32_t n, bool& irregular) {
    if (n == 0) return C_EMPTY;
    if (c0 == '+') {
        if (n > 1) irregular = true;
        return C_ABOVE;
    }
    if (c0 < '#') return C_BELOW;
    if (c0 < '+') return C_BETWEEN;
    return C_ABOVE;
}

// does the cuckoo key e (DictKey as uint4) hold the word of (head, n) whose
// bytes 8.. are p[8..n)?  (words over 8 bytes: the tail by id, then the arena)
template <class P>
__device__ __forceinline__ bool ck_match(const TokArgs& a, const uint4& e, uint64_t head, uint32_t n, P p) {
    if (e.z != n || e.x != (uint32_t)head || e.y != (uint32_t)(head >> 32)) return false;
    if (n <= 8) return true;
    const DictTail t = a.tails[e.w];
    uint64_t h2 = 0;
    for (uint32_t k = 8; k < 16 && k < n; ++k) h2 |= (uint64_t)p[k] << (8 * (k - 8));
    if (t.head2 != h2) return false;
    const uint8_t* q = a.arena + t.off;
    for (uint32_t k = 16; k < n; ++k)
        if (q[k] != p[k]) return false;
    return true;
}

// id of word p[0..n) in the device dictionary (W_UNKNOWN if absent); P is an
// LDS or global byte pointer
template <class P>
__device__ __forceinline__ uint32_t dict_find(const TokArgs& a, P p, uint32_t n) {
    uint32_t h32 = HW_SEED;
    for (uint32_t i = 0; i < n; i += 4) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4 && i + k < n; ++k) v |= (uint32_t)p[i + k] << (8 * k);
        h32 = hw_step(h32, v);
    }
    const uint32_t h = hw_final(h32, n), m = (uint32_t)a.dict_mask;
    uint64_t head = 0;
    for (uint32_t k = 0; k < 8 && k < n; ++k) head |= (uint64_t)p[k] << (8 * k);
    const uint4 e1 = *reinterpret_cast<const uint4*>(a.keys + (h & m));
    if (e1.w == 0) return W_UNKNOWN;   // slots never empty again once filled: absent
    if (ck_match(a, e1, head, n, p)) return e1.w;
    uint32_t g32 = HW_SEED2;
    for (uint32_t i = 0; i < n; i += 4) {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4 && i + k < n; ++k) v |= (uint32_t)p[i + k] << (8 * k);
        g32 = hw_step(g32, v);
    }
    const uint4 e2 = *reinterpret_cast<const uint4*>(a.keys + (hw_final(g32, n) & m));
    if (ck_match(a, e2, head, n, p)) return e2.w;
    return W_UNKNOWN;
}

// entry of the word p[0..n): class << 29 | id
template <class P>
__device__ __forceinline__ uint32_t word_entry(const TokArgs& a, P p, uint32_t n, bool& irregular) {
    const uint8_t c0 = n ? p[0] : 0;
    const uint32_t cls = tok_class(c0, n, irregular);
    uint32_t id;
    if (n == 0) id = W_EMPTY;
    else if (n == 1 && c0 == '+') id = W_PLUS;
    else if (n == 1 && c0 == '#') id = W_HASH;
    else id = dict_find(a, p, n);
    return (cls << WID_BITS) | id;
}

__device__ __forceinline__ void tok_append_slow(const TokArgs& a, bool slow, uint32_t t) {
    const uint64_t m = __ballot(slow);
    if (!m) return;
    uint32_t base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(a.d_nslow, (uint32_t)__popcll(m));
    base = __shfl(base, 0, 64);
    if (slow) a.slow_list[base + prefix_count(m)] = t;
}

// byte_eq's 0x80 flags of one dword -> 4 bits (byte j -> bit j)
__device__ __forceinline__ uint32_t gather4(uint32_t m) { return (((m >> 7) * 0x204081u) >> 21) & 0xFu; }

// '/' bytes of 16 bytes, byte j -> bit j
__device__ __forceinline__ uint32_t slash_mask16(const uint4& x) {
    return gather4(byte_eq(x.x, '/')) | (gather4(byte_eq(x.y, '/')) << 4) | (gather4(byte_eq(x.z, '/')) << 8) |
           (gather4(byte_eq(x.w, '/')) << 12);
}

constexpr uint32_t TOK_RUN = 63;   // tiles per count run (their 64 boundaries: one per lane)

// pass 1: words per tile = '/' bytes + topics.  Each wave takes a contiguous
// run of tiles (a slice of the grid's share, TOK_RUN at a time): their
// boundaries in one vector load, then the run's bytes streamed with four
// 16-B loads per lane in flight; each lane walks a cursor over the boundaries
// and adds its chunks' '/' counts to the tiles' LDS counters.  Block 0 also
// clears the launch's control words.
__global__ __launch_bounds__(64) void tm_tok_count(TokArgs a) {
    __shared__ uint64_t bnd[TOK_RUN + 1];
    __shared__ uint32_t cnt[TOK_RUN];
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x == 0) {   // the launch's control words (kernels after this one use them)
        if (lane < 2) a.d_nslow[lane] = 0;
        for (uint32_t i = lane; i < a.zero_words; i += 64) a.zero[i] = 0;
    }
    const uint32_t tt = a.tile_topics;
    if (a.d_n) {   // a device-counted batch: the tiles past its topics count 0 words (the scan covers the bound)
        const uint32_t nb = (a.n + tt - 1) / tt;
        a.n = *a.d_n;
        for (uint32_t i = (a.n + tt - 1) / tt + blockIdx.x * 64 + lane; i < nb; i += gridDim.x * 64) a.wcount[i] = 0;
    }
    const uint32_t ntiles = (a.n + tt - 1) / tt;
    const uint32_t per = (ntiles + gridDim.x - 1) / gridDim.x;
    const uint32_t first = blockIdx.x * per, last = min(first + per, ntiles);
    for (uint32_t run = first; run < last; run += TOK_RUN) {
        const uint32_t K = min(TOK_RUN, last - run);
        if (lane <= K) bnd[lane] = a.offs[min((run + lane) * tt, a.n)] - a.base;
        if (lane < K) cnt[lane] = 0;
        __syncthreads();
        const uint64_t B0 = bnd[0], BK = bnd[K], a0 = B0 & ~15ull;
        uint32_t j = 0;   // my cursor: the tile of my current chunk
        for (uint64_t p0 = a0 + 16u * lane; p0 < BK; p0 += 4096) {
            uint4 x[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint64_t p = p0 + 1024u * u;
                x[u] = p < BK ? *reinterpret_cast<const uint4*>(a.bytes + p) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) {
                const uint64_t p = p0 + 1024u * u;
                if (p >= BK) break;
                uint32_t m = slash_mask16(x[u]);
                if (p < B0) m &= ~0u << (uint32_t)(B0 - p);
                if (p + 16 > BK) m &= (1u << (uint32_t)(BK - p)) - 1u;
                while (j + 1 < K && bnd[j + 1] <= p) ++j;
                while (m) {   // bits up to the next boundary belong to tile j
                    const uint64_t lim = j + 1 < K ? bnd[j + 1] - p : 16u;
                    if (lim >= 16) {
                        atomicAdd(&cnt[j], (uint32_t)__popc(m));
                        break;
                    }
                    const uint32_t below = m & ((1u << (uint32_t)lim) - 1u);
                    if (below) atomicAdd(&cnt[j], (uint32_t)__popc(below));
                    m &= ~((1u << (uint32_t)lim) - 1u);
                    ++j;
                }
            }
        }
        __syncthreads();
        if (lane < K) {
            const uint32_t t0 = (run + lane) * tt;
            a.wcount[run + lane] = cnt[lane] + (min(t0 + tt, a.n) - t0);
        }
        __syncthreads();
    }
}

struct alignas(16) TokLds {
    uint8_t bytes[TOK_BYTES + 32];      // the tile's window; + 32: 8-byte reads past a word stay inside
    uint64_t tsb[TOK_BYTES / 64 + 1];   // topic-start bitmap of the window (+1: a lane's bits may straddle)
    uint16_t wst[TOK_WORDS];            // word start | 0x8000 when it is its topic's first word
    uint8_t wtop[TOK_WORDS];            // tile-local topic of each word
    uint32_t ttoff[TILE + 1];           // tile-local first word of each topic; [cnt] = words
    uint32_t tirr[TILE];                // a word of the topic starts with '+' but is not '+'
};

#ifndef TM_TOK_WPL
#define TM_TOK_WPL 2
#endif
constexpr uint32_t TOK_WPL_FILL = TM_TOK_WPL;   // words per lane per lookup round (register budget: occupancy)

// The tile's words w = lane + 64 k, TOK_WPL per lane at a time: start from
// wst, length from the next word's start (the last word of a topic ends at
// the next topic's start, others one byte ('/') before the next word), class
// and reserved atoms, then the dictionary: hash and head from LDS, every
// word's primary cuckoo slot loaded at once; the alternate slot only when the
// primary holds another word (cuckoo slots never empty again once filled, so
// an empty primary slot means the word is absent).  Lookups are bound by L2
// requests, not instructions: one per word is the point.
// Entries (class << 29 | id) go straight to words[].
template <uint32_t TOK_WPL>
__device__ __forceinline__ void tok_lookup(const TokArgs& a, TokLds& L, uint32_t tw, uint32_t wend,
                                           uint64_t tile_base, uint32_t* lw) {
    const uint32_t lane = threadIdx.x;
    const uint32_t mask = (uint32_t)a.dict_mask;
    for (uint32_t base = 0; base < tw; base += 64 * TOK_WPL) {
        uint64_t head[TOK_WPL];
        uint32_t ent[TOK_WPL], len[TOK_WPL], st[TOK_WPL], alt[TOK_WPL], pend = 0;
        uint4 e[TOK_WPL];
#pragma unroll
        for (uint32_t k = 0; k < TOK_WPL; ++k) {
            const uint32_t w = base + lane + 64 * k;
            const bool live = w < tw;
            // word bounds: start from wst, end at the next word's start (minus
            // the '/' unless the next word starts a topic)
            const uint32_t s0 = live ? L.wst[w] & 0x7FFFu : 0u;
            const uint32_t nx = live ? (w + 1 < tw ? L.wst[w + 1] : (wend | 0x8000u)) : 0x8000u;
            const uint32_t n = live ? (nx & 0x7FFFu) - s0 - ((nx & 0x8000u) ? 0u : 1u) : 0u;
            const uint64_t c0w = live ? lds_u64(L.bytes, s0) : 0ull;
            const uint32_t c0 = n ? (uint32_t)(c0w & 0xFF) : 0u;
            // class and reserved atoms, branch-free (emqx_topic:words/1's '' / '+' / '#')
            const uint32_t cls = n == 0 ? C_EMPTY : c0 < '#' ? C_BELOW : c0 < '+' ? C_BETWEEN : C_ABOVE;
            if (live && c0 == '+' && n > 1) L.tirr[L.wtop[w]] = 1;   // "+x": irregular topic
            const bool atom = n == 0 || (n == 1 && (c0 == '+' || c0 == '#'));
            ent[k] = (cls << WID_BITS) | (n == 0 ? W_EMPTY : c0 == '+' ? W_PLUS : W_HASH);
            len[k] = n;
            st[k] = s0;
            // both cuckoo hashes in one pass over the bytes (the mixing of
            // each 4-byte chunk is shared; only the accumulators differ)
            const uint64_t hd = low_bytes(c0w, n < 8 ? n : 8);
            uint32_t d = mix_chunk((uint32_t)hd);
            uint32_t h1 = hw_acc(HW_SEED, d), h2 = hw_acc(HW_SEED2, d);
            if (n > 4) {
                d = mix_chunk((uint32_t)(hd >> 32));
                h1 = hw_acc(h1, d);
                h2 = hw_acc(h2, d);
            }
            for (uint32_t i = 8; i < n; i += 8) {   // words over 8 bytes
                const uint64_t c = low_bytes(lds_u64(L.bytes, s0 + i), n - i < 8 ? n - i : 8);
                d = mix_chunk((uint32_t)c);
                h1 = hw_acc(h1, d);
                h2 = hw_acc(h2, d);
                if (n - i > 4) {
                    d = mix_chunk((uint32_t)(c >> 32));
                    h1 = hw_acc(h1, d);
                    h2 = hw_acc(h2, d);
                }
            }
            head[k] = hd;
            alt[k] = hw_final(h2, n) & mask;
            const bool look = live && !atom;
            e[k] = look ? *reinterpret_cast<const uint4*>(a.keys + (hw_final(h1, n) & mask)) : make_uint4(0, 0, 0, 0);
            pend |= look ? 1u << k : 0u;
        }
        // primary slots: a match or an empty slot settles the word
#pragma unroll
        for (uint32_t k = 0; k < TOK_WPL; ++k) {
            if (!(pend >> k & 1u)) continue;
            if (e[k].w == 0) {
                ent[k] = (ent[k] & ~WID_MASK) | W_UNKNOWN;
                pend &= ~(1u << k);
            } else if (ck_match(a, e[k], head[k], len[k], L.bytes + st[k])) {
                ent[k] = (ent[k] & ~WID_MASK) | e[k].w;
                pend &= ~(1u << k);
            }
        }
        // alternate slots of the rest, all in flight
#pragma unroll
        for (uint32_t k = 0; k < TOK_WPL; ++k)
            if (pend >> k & 1u) e[k] = *reinterpret_cast<const uint4*>(a.keys + alt[k]);
#pragma unroll
        for (uint32_t k = 0; k < TOK_WPL; ++k) {
            if (pend >> k & 1u)
                ent[k] = (ent[k] & ~WID_MASK) | (ck_match(a, e[k], head[k], len[k], L.bytes + st[k]) ? e[k].w : W_UNKNOWN);
            const uint32_t w = base + lane + 64 * k;
            if (w < tw && tile_base + w < a.words_cap) a.words[tile_base + w] = ent[k];
            if (lw && w < tw) lw[w] = ent[k];   // (the fused walk: the tile's words stay in LDS too)
        }
    }
}

// lane-per-topic path of a tile too long for the LDS budget: bytes from HBM
__device__ __forceinline__ uint8_t tok_fill_topic_global(const TokArgs& a, uint32_t t, uint64_t o, bool& slow) {
    const uint64_t b = a.offs[t] - a.base, e = a.offs[t + 1] - a.base;
    const uint8_t* p = a.bytes;
    bool irregular = false;
    uint32_t nw = 0;
    uint64_t ws = b;
    for (uint64_t i = b;; ++i) {
        if (i == e || p[i] == '/') {
            const uint32_t w = word_entry(a, p + ws, (uint32_t)(i - ws), irregular);
            if (o < a.words_cap) a.words[o] = w;
            ++o;
            ++nw;
            if (i == e) break;
            ws = i + 1;
        }
    }
    uint8_t fl = 0;
    if (e > b && p[b] == '$') fl |= TF_DOLLAR;
    if (irregular || nw > FAST_MAX_DEPTH) fl |= TF_SLOW;
    a.tflags[t] = fl;
    slow = (fl & TF_SLOW) != 0;
    return fl;
}

// One tokeniser tile (tm_tok_fill): words, offsets and flags to HBM, the
// generic-path list.
// out: per lane, its topic's first word (tile-local), word count and flags;
// lds = the tile went the LDS path (lw, if set, then holds its words).
struct TokTile {
    bool lds;
    uint32_t w0, nw;
    uint8_t fl;
    uint64_t base;   // the tile's first word in words[]
};
// (WPL: words per lane per lookup round -- the fused walk's register budget is tighter)
template <uint32_t WPL>
__device__ __forceinline__ void tok_tile(const TokArgs& a, TokLds& L, uint32_t tile, uint32_t* lw, TokTile& out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t tt = a.tile_topics;
    const uint32_t t0 = tile * tt, tend = min(t0 + tt, a.n), cnt = tend - t0;
    const uint32_t t = t0 + lane;
    const bool valid = lane < cnt;
    const uint64_t b0 = a.offs[t0] - a.base, b1 = a.offs[tend] - a.base;
    const uint64_t my_b = valid ? a.offs[t] - a.base : 0, my_e = valid ? a.offs[t + 1] - a.base : 0;
    const uint64_t a0 = b0 & ~15ull;   // bytes[] is 16-B aligned: so are the window's loads
    const uint64_t tile_base = (uint64_t)a.wcount[tile] + a.bsums[tile / SCAN_TILE];   // block-local scan + block offset
    bool slow = false;
    // the LDS path: the window fits and no topic is empty (an empty topic
    // starts where the next one does: one bit cannot mark both)
    bool lds = b1 - a0 <= TOK_BYTES && !__any(valid && my_b == my_e);
    uint32_t tw = 0, wend = 0, incl = 0, mine = 0;
    uint64_t S = 0, TS = 0;
    const uint32_t lb = lane * TOK_LANE_BYTES;   // my 48 bytes of the window
    out.base = tile_base;
    out.fl = (uint8_t)TF_SLOW;
    out.w0 = out.nw = 0;
    if (lds) {
        wend = (uint32_t)(b1 - a0);
        const uint32_t r0 = (uint32_t)(b0 - a0);
        uint4 v[TOK_LANE_BYTES / 16];
#pragma unroll
        for (uint32_t k = 0; k < TOK_LANE_BYTES / 16; ++k)
            v[k] = lb + 16 * k < wend ? *reinterpret_cast<const uint4*>(a.bytes + a0 + lb + 16 * k)
                                      : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (uint32_t k = 0; k < TOK_LANE_BYTES / 16; ++k)
            *reinterpret_cast<uint4*>(L.bytes + lb + 16 * k) = v[k];
        for (uint32_t i = lane; i < 2 * (TOK_BYTES / 64 + 1); i += 64) reinterpret_cast<uint32_t*>(L.tsb)[i] = 0u;
        if (lane < TILE) L.tirr[lane] = 0;
        __syncthreads();
        if (valid) {
            const uint32_t p = (uint32_t)(my_b - a0);
            atomicOr(reinterpret_cast<unsigned long long*>(&L.tsb[p >> 6]), 1ull << (p & 63));
        }
        // '/' bytes of my 48 (inside [r0, wend)) and topic starts, as bit masks
#pragma unroll
        for (uint32_t k = 0; k < TOK_LANE_BYTES / 16; ++k) {
            S |= (uint64_t)gather4(byte_eq(v[k].x, '/')) << (16 * k);
            S |= (uint64_t)gather4(byte_eq(v[k].y, '/')) << (16 * k + 4);
            S |= (uint64_t)gather4(byte_eq(v[k].z, '/')) << (16 * k + 8);
            S |= (uint64_t)gather4(byte_eq(v[k].w, '/')) << (16 * k + 12);
        }
        const uint32_t lo = r0 > lb ? min(r0 - lb, TOK_LANE_BYTES) : 0u;
        const uint32_t hi = wend > lb ? min(wend - lb, TOK_LANE_BYTES) : 0u;
        S &= ((1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
        __syncthreads();
        const uint32_t q = lb >> 6, sh = lb & 63;
        TS = L.tsb[q] >> sh;
        if (sh) TS |= L.tsb[q + 1] << (64 - sh);
        TS &= (1ull << TOK_LANE_BYTES) - 1ull;
        // word starts = topic starts + '/' bytes; one scan numbers them
        mine = (uint32_t)(__popcll(S) + __popcll(TS)) | ((uint32_t)__popcll(TS) << 16);
        incl = mine;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, 64);
            if (lane >= (uint32_t)o) incl += u;
        }
        tw = __shfl(incl, 63, 64) & 0xFFFFu;
        if (tw > TOK_WORDS) {
            lds = false;
            __syncthreads();
        }
    }
    uint32_t nw = 0, tincl = 0;
    if (!lds) {
        // long tile: one lane per topic, bytes from HBM; in-tile offsets by
        // a wave scan of the per-topic word counts ('/' + 1)
        if (valid) {
            nw = 1;
            for (uint64_t i = my_b; i < my_e; ++i) nw += a.bytes[i] == '/';
        }
        tincl = nw;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = __shfl_up(tincl, o, 64);
            if (lane >= (uint32_t)o) tincl += u;
        }
        tw = __shfl(tincl, 63, 64);
    }
    if (tend == a.n && lane == 0) a.toff[a.n] = (uint32_t)(tile_base + tw);
    out.lds = lds;
    if (lds) {
        uint32_t wi = (incl - mine) & 0xFFFFu;            // my first word
        int32_t tc = (int32_t)((incl - mine) >> 16) - 1;   // the topic my first byte is in
        uint64_t m = S | TS;
        while (m) {
            const uint32_t b = (uint32_t)__builtin_ctzll(m);
            m &= m - 1;
            const uint32_t pos = lb + b;
            if (TS >> b & 1ull) {
                ++tc;
                L.ttoff[tc] = wi;
                L.wst[wi] = (uint16_t)(pos | 0x8000u);
                L.wtop[wi++] = (uint8_t)tc;
            }
            if (S >> b & 1ull) {
                L.wst[wi] = (uint16_t)(pos + 1);
                L.wtop[wi++] = (uint8_t)tc;
            }
        }
        if (lane == 0) L.ttoff[cnt] = tw;
        __syncthreads();
        tok_lookup<WPL>(a, L, tw, wend, tile_base, lw);   // the tile's words, round-robin over lanes
        __syncthreads();
        if (valid) {
            const uint32_t w0 = L.ttoff[lane], tn = L.ttoff[lane + 1] - w0;
            uint8_t fl = 0;
            if (L.bytes[my_b - a0] == '$') fl |= TF_DOLLAR;
            if (L.tirr[lane] || tn > FAST_MAX_DEPTH) fl |= TF_SLOW;
            a.tflags[t] = fl;
            a.toff[t] = (uint32_t)(tile_base + w0);
            slow = (fl & TF_SLOW) != 0;
            out.w0 = w0;
            out.nw = tn;
            out.fl = fl;
        }
        tok_append_slow(a, slow, t);
        __syncthreads();
    } else {
        const uint64_t o = tile_base + tincl - nw;
        if (valid) {
            a.toff[t] = (uint32_t)o;
            out.fl = tok_fill_topic_global(a, t, o, slow);
            out.w0 = tincl - nw;
            out.nw = nw;
        }
        tok_append_slow(a, slow, t);
    }
}

// pass 2 (after the scan of the tile counts): word entries, offsets, flags
#ifndef TM_TOK_WPE
#define TM_TOK_WPE 5
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(TM_TOK_WPE, 8))) void tm_tok_fill(TokArgs a) {
    __shared__ TokLds L;
    if (a.d_n) a.n = *a.d_n;   // a device-counted batch (its bound sized the grid and the scan)
    const uint32_t tt = a.tile_topics;
    const uint32_t ntiles = (a.n + tt - 1) / tt;
    TokTile out;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) tok_tile<TOK_WPL_FILL>(a, L, tile, nullptr, out);
}


// Read-back of an async batch in ONE kernel, written straight into pinned host
// memory: the header block's first hdr_words (ctrl + stats + src), the counts,
// and exactly the staging entries the walk reserved (ctrl's u64 ticket; the
// host checks it against rows_cap) -- instead of three DMA copies, one of them
// sized by a guess.
__global__ __launch_bounds__(256) void tm_export_host(ExportArgs a) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t i0 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (a.d_n) {   // a bounded batch: the layout follows its count
        a.n = *a.d_n;
        a.hdr_words = a.fixed_words + 2 * a.n;
        a.h_count = a.h_hdr + a.hdr_words;
    }
    for (uint64_t i = i0; i < a.hdr_words; i += stride) a.h_hdr[i] = a.hdr[i];
    for (uint64_t i = i0; i < a.n; i += stride) a.h_count[i] = a.count[i];
    for (uint32_t g = 0; g < TICKET_GROUPS; ++g) {   // each group region's reserved entries
        const uint64_t top = xg_top_read(a.hdr, g);
        const uint64_t lo = g * a.rcap, hi = lo + (top < a.rcap ? top : a.rcap);
        for (uint64_t i = lo + i0; i < hi && i < a.rows_cap; i += stride) a.h_rows[i] = a.rows[i];
    }
}

__global__ __launch_bounds__(256) void tm_csr_to_host(const uint32_t* row_off, const uint32_t* ids, uint32_t n,
                                                       const uint32_t* d_total, uint64_t cap, uint32_t* h_row,
                                                       uint32_t* h_ids) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const uint64_t i0 = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = min((uint64_t)*d_total, cap);
    for (uint64_t i = i0; i <= n; i += stride) h_row[i] = row_off[i];
    for (uint64_t i = i0; i < total; i += stride) h_ids[i] = ids[i];
}

hipError_t launch_csr_to_host(const uint32_t* row_off, const uint32_t* ids, uint32_t n, const uint32_t* d_total,
                              uint64_t cap, uint32_t* h_row, uint32_t* h_ids, hipStream_t s) {
    const uint64_t work = std::max<uint64_t>(cap, (uint64_t)n + 1);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((work / 8 + 255) / 256, 1), 1024);
    hipLaunchKernelGGL(tm_csr_to_host, dim3(grid), dim3(256), 0, s, row_off, ids, n, d_total, cap, h_row, h_ids);
    return hipGetLastError();
}

// 4 ids -> 12 bytes (three aligned dword stores) per thread; the last
// partial group byte by byte
__global__ __launch_bounds__(256) void tm_pack_ids(const uint32_t* ids, uint64_t n, uint8_t* out) {
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x, j = 4 * g;
    if (j >= n) return;
    if (j + 4 <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(ids + j);
        uint32_t* o = reinterpret_cast<uint32_t*>(out + 12 * g);
        o[0] = (v.x & 0xFFFFFFu) | (v.y << 24);
        o[1] = ((v.y >> 8) & 0xFFFFu) | (v.z << 16);
        o[2] = ((v.z >> 16) & 0xFFu) | (v.w << 8);
        return;
    }
    for (uint64_t q = j; q < n; ++q)
        for (uint32_t b = 0; b < 3; ++b) out[3 * q + b] = (uint8_t)(ids[q] >> (8 * b));
}

hipError_t launch_pack_ids(const uint32_t* ids, uint64_t n, uint8_t* out, hipStream_t s) {
    const uint64_t groups = (n + 3) / 4;
    if (groups) hipLaunchKernelGGL(tm_pack_ids, dim3((uint32_t)((groups + 255) / 256)), dim3(256), 0, s, ids, n, out);
    return hipGetLastError();
}

hipError_t launch_export_host(const ExportArgs& a, hipStream_t s) {
    const uint64_t work = a.hdr_words + a.n + a.rows_cap;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((work / 4 + 255) / 256, 1), 512);
    hipLaunchKernelGGL(tm_export_host, dim3(grid), dim3(256), 0, s, a);
    return hipGetLastError();
}

__global__ void tm_scatter_keys(DictKey* keys, const uint32_t* idx, const DictKey* vals, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[idx[i]] = vals[i];
}

// ------------------------------------------------------------ launchers

// Topics per tile: 64 (one per lane) for large batches; small batches use
// fewer per wave so that they spread over >= ~2048 waves -- a tile's latency
// is its probe count / 64 iterations, so one topic per wave walks in about
// depth dependent rounds instead of the 64 topics' combined frontier.
#ifndef TM_MIN_TILES
#define TM_MIN_TILES 256    // small batches: tiles shrink until there are this many (4,096-topic batch p50: 2048 / 1024 / 512 / 256 / 128 -> 0.16 / 0.10 / 0.07 / 0.063 / 0.082 ms)
#endif
uint32_t tile_topics(uint32_t n) {
    uint32_t tt = 64;
    while (tt > 1 && (n + tt - 1) / tt < TM_MIN_TILES) tt >>= 1;
    return tt;
}

uint32_t match_waves(uint32_t n, int device, uint32_t qcap) {
    static uint32_t cap[64][2] = {};
    const int qi = qcap <= 384 ? 0 : 1;
    const uint32_t tt = tile_topics(n);
    const uint32_t ntiles = (n + tt - 1) / tt;
    uint32_t c = (device >= 0 && device < 64) ? cap[device][qi] : 0u;
    if (!c) {
        int per_cu = 0, cus = 0;
        // the four instances of one stack size share its LDS footprint, which bounds residency
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_cu, qi == 0 ? tm_match_tiles<false, false, 384> : tm_match_tiles<false, false, 512>, 64, 0) !=
                hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
            per_cu <= 0 || cus <= 0) {
            (void)hipGetLastError();
            per_cu = qi == 0 ? 16 : 14;
            cus = 256;
        }
        // TM_WAVES_PER_CU: fewer resident waves (occupancy sweeps in tools/; never more than fit)
        if (const char* w = getenv("TM_WAVES_PER_CU")) per_cu = std::min(per_cu, std::max(1, atoi(w)));
        c = (uint32_t)per_cu * (uint32_t)cus;
        if (device >= 0 && device < 64) cap[device][qi] = c;
    }
    return ntiles < c ? ntiles : c;
}

template <bool CK, bool BIG>
static hipError_t launch_match_t(const MatchArgs& a, hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b,
                                 unsigned ev_flags) {
    const uint32_t ntiles = (a.n + a.tile_topics - 1) / a.tile_topics;
    hipError_t e;
    if (ev_a && (e = hipEventRecordWithFlags(ev_a, s, ev_flags)) != hipSuccess) return e;
    if (ntiles) {
        const uint32_t grid = a.grid;
        if (a.qcap <= 384) hipLaunchKernelGGL((tm_match_tiles<CK, BIG, 384>), dim3(grid), dim3(64), 0, s, a);
        else hipLaunchKernelGGL((tm_match_tiles<CK, BIG, 512>), dim3(grid), dim3(64), 0, s, a);
    }
    if (ev_b && (e = hipEventRecordWithFlags(ev_b, s, ev_flags)) != hipSuccess) return e;
    if (ntiles && a.wstats) hipLaunchKernelGGL(tm_stats_reduce, dim3(1), dim3(256), 0, s, a.wstats, a.grid, a.stats);
    hipLaunchKernelGGL((tm_match_slow<CK, BIG>), dim3(a.s_waves), dim3(64), 0, s, a);
    return hipSuccess;
}

// ev_flags: hipEventRecordExternal while the stream is being captured into a
// graph, so that every replay re-records the timing events (a plain record in
// a capture only adds a dependency, and the events would keep the times of the
// last direct launch)
hipError_t launch_match(const MatchArgs& a, hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b, bool checked,
                        unsigned ev_flags) {
    // the edge hash is read with 32-bit-offset buffer loads unless it exceeds
    // 4 GiB less a bucket: the walk's lanes without a probe read at OFF_NONE,
    // which has to lie past the table (nslots * 16 + 64 <= 2^32)
    const bool big = (uint64_t)a.nslots * sizeof(Slot) > (uint64_t)OFF_NONE;
    hipError_t e;
    if (checked) e = big ? launch_match_t<true, true>(a, s, ev_a, ev_b, ev_flags)
                         : launch_match_t<true, false>(a, s, ev_a, ev_b, ev_flags);
    else e = big ? launch_match_t<false, true>(a, s, ev_a, ev_b, ev_flags)
                 : launch_match_t<false, false>(a, s, ev_a, ev_b, ev_flags);
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

hipError_t launch_scan(const ScanArgs& a, hipStream_t s, uint32_t* d_total) {
    const uint32_t nb = scan_block_count(a.n);
    if (nb <= 1) {
        hipLaunchKernelGGL(tm_scan_local, dim3(1), dim3(SCAN_BLOCK), 0, s, a, d_total);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(tm_scan_local, dim3(nb), dim3(SCAN_BLOCK), 0, s, a, (uint32_t*)nullptr);
    hipLaunchKernelGGL(tm_scan_sums, dim3(1), dim3(SCAN_BLOCK), 0, s, a, nb, d_total);
    return hipGetLastError();
}

hipError_t launch_finalize(const ScanArgs& a, hipStream_t s, bool checked) {
    const uint32_t ntiles = (a.n + TILE - 1) / TILE;
    if (!ntiles) return hipGetLastError();
    const uint32_t grid = min(ntiles, 256u * 32u);   // 8 waves per SIMD
    if (checked) hipLaunchKernelGGL(tm_finalize<true>, dim3(grid), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(tm_finalize<false>, dim3(grid), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shared_count(const SharedArgs& a, hipStream_t s) {
    if (a.m) hipLaunchKernelGGL(tm_shared_count, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shared_rows(const SharedArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tm_shared_rows, dim3((a.n + 1 + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shared_pick(const SharedArgs& a, hipStream_t s) {
    if (a.m) hipLaunchKernelGGL(tm_shared_pick, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shared_fold(SharedSlot* slots, const uint2* upd, uint32_t nslots, hipStream_t s) {
    if (nslots) hipLaunchKernelGGL(tm_shared_fold, dim3((nslots + 255) / 256), dim3(256), 0, s, slots, upd, nslots);
    return hipGetLastError();
}

hipError_t launch_route_count(const RouteArgs& a, hipStream_t s) {
    if (a.m) hipLaunchKernelGGL(tm_route_count, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_rows(const RouteArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tm_route_rows, dim3((a.n + 1 + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_fill(const RouteArgs& a, hipStream_t s) {
    if (a.m) hipLaunchKernelGGL(tm_route_fill, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fan_scan(const FanArgs& a, hipStream_t s) {
    const uint64_t ne = a.n_matches + 1;
    const uint32_t nb = (uint32_t)((ne + FAN_SCAN_TILE - 1) / FAN_SCAN_TILE);
    hipLaunchKernelGGL(tm_fan_scan_local, dim3(nb), dim3(FAN_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tm_fan_scan_sums, dim3(1), dim3(FAN_BLOCK), 0, s, a, nb);
    if (a.nreg) {
        if (a.n) hipLaunchKernelGGL(tm_fan_rows_stg, dim3((a.n + FAN_BLOCK - 1) / FAN_BLOCK), dim3(FAN_BLOCK), 0, s, a);
    } else {
        hipLaunchKernelGGL(tm_fan_rows, dim3((a.n + 1 + FAN_BLOCK - 1) / FAN_BLOCK), dim3(FAN_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_fan_globalize(const FanArgs& a, hipStream_t s) {
    const uint64_t ne = a.n_matches + 1;
    hipLaunchKernelGGL(tm_fan_scan_add, dim3((uint32_t)((ne + FAN_BLOCK - 1) / FAN_BLOCK)), dim3(FAN_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_fan_fill(const FanArgs& a, hipStream_t s) {
    if (a.total) {
        const uint64_t nt = (a.total + FAN_FILL_TILE - 1) / FAN_FILL_TILE;
        hipLaunchKernelGGL(tm_fan_tiles, dim3((uint32_t)((nt + 1 + FAN_BLOCK - 1) / FAN_BLOCK)), dim3(FAN_BLOCK), 0, s,
                           a, nt);
        if (a.out_j) {
            if (a.total > a.big_limit) hipLaunchKernelGGL((tm_fan_fill<true, true>), dim3((uint32_t)nt), dim3(FAN_BLOCK), 0, s, a);
            else hipLaunchKernelGGL((tm_fan_fill<false, true>), dim3((uint32_t)nt), dim3(FAN_BLOCK), 0, s, a);
        } else if (a.total > a.big_limit) hipLaunchKernelGGL(tm_fan_fill<true>, dim3((uint32_t)nt), dim3(FAN_BLOCK), 0, s, a);
        else hipLaunchKernelGGL(tm_fan_fill<false>, dim3((uint32_t)nt), dim3(FAN_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_inbox_pubof(const InboxArgs& a, hipStream_t s) {
    if (a.m && a.n) hipLaunchKernelGGL(tm_inbox_pubof, dim3((a.m + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_inbox_sort(const InboxArgs& a, hipStream_t s) {
    if (!a.D || !a.ntiles || a.passes > INBOX_MAX_PASSES) return hipGetLastError();
    ScanArgs sa{};
    sa.count = a.hist; sa.row_off = a.hist; sa.block_sums = a.hbs; sa.n = 256u * a.ntiles;   // in place
    for (uint32_t p = 0; p < a.passes; ++p) {
        const uint32_t* kin = p & 1 ? a.key1 : a.key0;
        const uint32_t* vin = p & 1 ? a.val1 : a.val0;
        uint32_t* kout = p & 1 ? a.key0 : a.key1;
        uint32_t* vout = p & 1 ? a.val0 : a.val1;
        hipLaunchKernelGGL(tm_inbox_hist, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a, kin, a.hist, 8 * p);
        const hipError_t e = launch_scan(sa, s, nullptr);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(tm_inbox_scatter, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a, kin, vin, kout, vout,
                           (const uint32_t*)a.hist, (const uint32_t*)a.hbs, 8 * p);
    }
    return hipGetLastError();
}

hipError_t launch_inbox_merge(const MergeArgs& a, hipStream_t s) {
    const uint64_t tot = (uint64_t)a.nd + a.ns;
    if (tot) hipLaunchKernelGGL(tm_inbox_merge, dim3((uint32_t)((tot + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_inbox_finish(const InboxArgs& a, hipStream_t s) {
    if (!a.D || !a.ntiles) return hipGetLastError();
    const uint32_t* keys = a.passes & 1 ? a.key1 : a.key0;
    const uint32_t* vals = a.passes & 1 ? a.val1 : a.val0;
    if (a.mrec) hipLaunchKernelGGL(tm_inbox_finish<true>, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a, keys, vals);
    else hipLaunchKernelGGL(tm_inbox_finish<false>, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a, keys, vals);
    ScanArgs sa{};
    sa.count = a.hcount; sa.row_off = a.hcount; sa.block_sums = a.hcbs; sa.n = a.ntiles;   // in place
    const hipError_t e = launch_scan(sa, s, a.d_R);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tm_inbox_heads, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a, keys);
    return hipGetLastError();
}

hipError_t launch_deliver_flags(const DeliverArgs& a, bool drop, hipStream_t s) {
    if (!a.D || !a.R || !a.ntiles) return hipGetLastError();
    hipLaunchKernelGGL(tm_deliver_range, dim3((a.R + 255) / 256), dim3(256), 0, s, a);
    if (a.groups) {
        if (drop)
            hipLaunchKernelGGL((tm_deliver_flags<true, true>), dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a);
        else
            hipLaunchKernelGGL((tm_deliver_flags<false, true>), dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a);
    } else if (drop)
        hipLaunchKernelGGL((tm_deliver_flags<true, false>), dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL((tm_deliver_flags<false, false>), dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_deliver_compact(const DeliverArgs& a, hipStream_t s) {
    if (!a.D || !a.R || !a.ntiles) return hipGetLastError();
    hipLaunchKernelGGL(tm_deliver_count, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a);
    ScanArgs sk{}, sn{};
    sk.count = a.kcount; sk.row_off = a.kcount; sk.block_sums = a.kbs; sk.n = a.ntiles;   // in place
    sn.count = a.ncount; sn.row_off = a.ncount; sn.block_sums = a.nbs; sn.n = a.ntiles;
    hipError_t e = launch_scan(sk, s, a.d_tot);
    if (e != hipSuccess) return e;
    if ((e = launch_scan(sn, s, a.d_tot + 1)) != hipSuccess) return e;
    if (a.groups) hipLaunchKernelGGL(tm_deliver_scatter<true>, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a);
    else hipLaunchKernelGGL(tm_deliver_scatter<false>, dim3(a.ntiles), dim3(INBOX_BLOCK), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_window(const WindowArgs& a, hipStream_t s) {
    if (!a.D || !a.R || !a.nwaves) return hipGetLastError();
    const uint32_t ntiles = a.nwaves / (INBOX_BLOCK / 64);
    hipLaunchKernelGGL(tm_window_state, dim3((a.R + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_window_count, dim3(ntiles), dim3(INBOX_BLOCK), 0, s, a);
    ScanArgs sc{};
    sc.count = a.wcount; sc.row_off = a.wcount; sc.block_sums = a.wbs; sc.n = a.nwaves;   // in place
    const hipError_t e = launch_scan(sc, s, a.d_tot);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tm_window_plan, dim3((a.R + 255) / 256), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_window_classify, dim3(ntiles), dim3(INBOX_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tm_window_totals, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_prio_lookup(const PrioLookupArgs& a, hipStream_t s) {
    if (a.n && a.ntab) hipLaunchKernelGGL(tm_prio_lookup, dim3((a.n + 255) / 256, a.ntab), dim3(256), 0, s, a);
    return hipGetLastError();
}

// launch_window's sequence with the class kernels in it: the session's table
// needs tm_window_state's flags and M, the class counts need the old plan's nsend
hipError_t launch_window_prio(const WindowArgs& a, const PrioArgs& p, hipStream_t s) {
    if (!a.D || !a.R || !a.nwaves) return hipGetLastError();
    const uint32_t ntiles = a.nwaves / (INBOX_BLOCK / 64), rblocks = (a.R + 255) / 256;
    const uint32_t nsb = (a.nwaves + PRIO_SCAN_TILE - 1) / PRIO_SCAN_TILE;
    hipLaunchKernelGGL(tm_window_state, dim3(rblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_winp_session, dim3(rblocks), dim3(256), 0, s, a, p);
    hipLaunchKernelGGL(tm_window_count, dim3(ntiles), dim3(INBOX_BLOCK), 0, s, a);
    ScanArgs sc{};
    sc.count = a.wcount; sc.row_off = a.wcount; sc.block_sums = a.wbs; sc.n = a.nwaves;   // in place
    const hipError_t e = launch_scan(sc, s, a.d_tot);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tm_window_plan, dim3(rblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_winp_count, dim3(ntiles), dim3(INBOX_BLOCK), 0, s, a, p);
    hipLaunchKernelGGL(tm_winp_scan_tiles, dim3(nsb), dim3(256), 0, s, p, a.nwaves);
    hipLaunchKernelGGL(tm_winp_scan_sums, dim3(1), dim3(64), 0, s, p, nsb);
    hipLaunchKernelGGL(tm_winp_plan, dim3(rblocks), dim3(256), 0, s, a, p);
    hipLaunchKernelGGL(tm_winp_classify, dim3(ntiles), dim3(INBOX_BLOCK), 0, s, a, p);
    hipLaunchKernelGGL(tm_window_totals, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_drain(const DrainArgs& a, hipStream_t s) {
    if (!a.Q || !a.R || !a.nwaves) return hipGetLastError();
    const uint32_t ntiles = a.nwaves / (INBOX_BLOCK / 64), rblocks = (a.R + 255) / 256;
    const uint32_t nsb = (a.nwaves + PRIO_SCAN_TILE - 1) / PRIO_SCAN_TILE;
    hipLaunchKernelGGL(tm_drain_heads, dim3(rblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_drain_count, dim3(ntiles), dim3(INBOX_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tm_drain_scan_tiles, dim3(nsb, DRAIN_PLANES), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_drain_scan_sums, dim3(1), dim3(64), 0, s, a, nsb);
    hipLaunchKernelGGL(tm_drain_plan, dim3(rblocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_drain_classify, dim3(ntiles), dim3(INBOX_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tm_drain_totals, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

uint32_t fan_scan_tile() { return FAN_SCAN_TILE; }
uint32_t fan_fill_tile() { return FAN_FILL_TILE; }

hipError_t launch_rules_match(const RulesArgs& a, hipStream_t s) {
    if (a.n) hipLaunchKernelGGL(tm_rules_match, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_acl_check(const AclArgs& a, hipStream_t s) {
    if (a.n) hipLaunchKernelGGL(tm_acl_check, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_gather_rows(const uint32_t* src, const int64_t* src_off, const int64_t* idx, uint32_t n,
                              const int64_t* dst_off, uint32_t* dst, hipStream_t s) {
    if (n) hipLaunchKernelGGL(tm_gather_rows, dim3((uint32_t)(((uint64_t)n * 16 + 255) / 256)), dim3(256), 0, s, src,
                              src_off, idx, n, dst_off, dst);
    return hipGetLastError();
}

hipError_t launch_dedup(const DedupArgs& a, ScanArgs rows_scan, ScanArgs bytes_scan, hipStream_t s) {
    if (!a.n) return hipGetLastError();
    const uint32_t nblk = dedup_blocks(a.n);
    hipLaunchKernelGGL(tm_dedup_claim, dim3((a.n + DD_BLOCK - 1) / DD_BLOCK), dim3(DD_BLOCK), 0, s, a);
    hipLaunchKernelGGL(tm_dedup_count, dim3(nblk), dim3(256), 0, s, a);
    hipError_t e;
    if ((e = launch_scan(rows_scan, s, nullptr)) != hipSuccess) return e;
    if ((e = launch_scan(bytes_scan, s, nullptr)) != hipSuccess) return e;
    hipLaunchKernelGGL(tm_dedup_compact, dim3(nblk), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dedup_rowof(const DedupArgs& a, hipStream_t s) {
    if (a.n) hipLaunchKernelGGL(tm_dedup_rowof, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_dedup_expand(const DedupArgs& a, hipStream_t s) {
    const uint32_t g = (a.n + 256 * EXPAND_PER_THREAD - 1) / (256 * EXPAND_PER_THREAD);
    // (the rows are counted on the device: a grid for the bound, strided)
    const uint32_t gr = std::min<uint32_t>(2048, (a.n + 255) / 256);
    if (gr) hipLaunchKernelGGL(tm_dedup_rowmeta, dim3(gr), dim3(256), 0, s, a);
    if (g) hipLaunchKernelGGL(tm_dedup_expand, dim3(g), dim3(256), 0, s, a);
    hipLaunchKernelGGL(tm_dedup_sum, dim3(1), dim3(1024), 0, s, a, g);   // (also reports the rows)
    return hipGetLastError();
}

hipError_t launch_sample_meta(const uint32_t* count, const unsigned long long* src, const uint32_t* rows, uint32_t k,
                              uint32_t* out_cnt, unsigned long long* out_src, hipStream_t s) {
    if (k) hipLaunchKernelGGL(tm_sample_meta, dim3((k + 255) / 256), dim3(256), 0, s, count, src, rows, k, out_cnt, out_src);
    return hipGetLastError();
}

hipError_t launch_sample_ids(const uint32_t* sfids, const uint32_t* cnt, const unsigned long long* src,
                             const uint64_t* off, uint32_t k, uint32_t* out, hipStream_t s) {
    if (k) hipLaunchKernelGGL(tm_sample_ids, dim3(k), dim3(64), 0, s, sfids, cnt, src, off, out);
    return hipGetLastError();
}

hipError_t launch_token_check(const uint32_t* toff, const uint8_t* tflags, uint32_t n, uint64_t nwords,
                              uint32_t* slow_list, uint32_t* d_nslow, uint32_t* d_bad, hipStream_t s) {
    if (n) hipLaunchKernelGGL(tm_token_check, dim3((n + 255) / 256), dim3(256), 0, s, toff, tflags, n, nwords,
                              slow_list, d_nslow, d_bad);
    return hipGetLastError();
}

hipError_t launch_tokens_shard(const uint32_t* words, const uint32_t* toff, uint32_t n, uint32_t nshards,
                               uint32_t* shard, hipStream_t s) {
    if (n) hipLaunchKernelGGL(tm_tokens_shard, dim3((n + 255) / 256), dim3(256), 0, s, words, toff, n, nshards, shard);
    return hipGetLastError();
}

hipError_t launch_part_count(const PartArgs& a, hipStream_t s) {
    if (a.n) hipLaunchKernelGGL(tm_part_count, dim3(a.nb), dim3(PART_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_part_segs(const PartArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(tm_part_segs, dim3(1), dim3(PART_MAX_G + 1), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_part_scatter(const PartArgs& a, hipStream_t s) {
    if (a.n) hipLaunchKernelGGL(tm_part_scatter, dim3(a.nb), dim3(PART_BLOCK), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_unpart_counts(const uint32_t* order, const uint32_t* counts_p, uint32_t n, uint32_t* counts_o,
                                hipStream_t s) {
    if (n) hipLaunchKernelGGL(tm_unpart_counts, dim3((n + 255) / 256), dim3(256), 0, s, order, counts_p, n, counts_o);
    return hipGetLastError();
}
hipError_t launch_unpart_rows(const uint32_t* order, const uint32_t* counts_p, uint32_t n, const uint32_t* src_off,
                              const uint32_t* src_bs, const uint32_t* dst_off, const uint32_t* dst_bs,
                              const uint32_t* ids_p, uint32_t* out, uint32_t* rowg, hipStream_t s) {
    const uint64_t threads = ((uint64_t)n + 1) * 16;
    hipLaunchKernelGGL(tm_unpart_rows, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, order, counts_p, n,
                       src_off, src_bs, dst_off, dst_bs, ids_p, out, rowg);
    return hipGetLastError();
}

hipError_t launch_export(const uint32_t* row_off, const uint32_t* ids, uint32_t n, uint64_t total,
                         uint32_t* counts, uint32_t* gids, uint32_t mul, uint32_t add, hipStream_t s) {
    const uint64_t work = total > n ? total : n;
    if (!work) return hipGetLastError();
    const uint64_t blocks = (work + 255) / 256;
    const uint32_t grid = (uint32_t)(blocks < 4096u ? blocks : 4096u);
    hipLaunchKernelGGL(tm_export, dim3(grid), dim3(256), 0, s, row_off, ids, n, total, counts, gids, mul, add);
    return hipGetLastError();
}

hipError_t launch_scatter_slots(Slot* slots, const uint32_t* idx, const Slot* vals, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(tm_scatter_slots, dim3((n + 255) / 256), dim3(256), 0, s, slots, idx, vals, n);
    return hipGetLastError();
}

hipError_t launch_scatter_fmeta(uint64_t* foff, uint32_t* flen, const uint32_t* idx, const uint64_t* off,
                                const uint32_t* len, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(tm_scatter_fmeta, dim3((n + 255) / 256), dim3(256), 0, s, foff, flen, idx, off, len, n);
    return hipGetLastError();
}

uint32_t tok_tile_topics(uint32_t n, uint64_t nbytes) {
    // the most topics (64 at most) whose average bytes fill ~3/4 of the LDS window
    uint32_t tt = TILE;
    while (tt > 1 && (uint64_t)tt * nbytes > (uint64_t)(TOK_BYTES * 3 / 4) * (n ? n : 1)) tt >>= 1;
    // small batches (per-publish calls): at least 32 tiles down to 4 topics a
    // tile -- one wave walking a whole 64-topic tile's lookups is a chain of
    // dependent rounds; several short tiles run them side by side
    while (tt > 4 && (n + tt - 1) / tt < 32) tt >>= 1;
    return tt;
}

// blocks of `kernel` (block threads, no dynamic LDS) the device holds at once:
// a grid of that size runs in one round (no tail of late blocks)
template <class K>
static uint32_t resident_blocks(K kernel, int block) {
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, block, 0) != hipSuccess || cus <= 0 || per <= 0)
        return 256u * 32u;
    return (uint32_t)(cus * per);
}

// tokeniser passes 1 and 2: words per tile, their scan (f: the fill's arguments)
static hipError_t launch_tok_count_scan(const TokArgs& a, ScanArgs scan, uint32_t* d_nwords, hipStream_t s,
                                        TokArgs& f) {
    static const uint32_t cap_count = resident_blocks(tm_tok_count, 64);
    const uint32_t ntiles = (a.n + a.tile_topics - 1) / a.tile_topics;
    hipLaunchKernelGGL(tm_tok_count, dim3(ntiles ? min(ntiles, cap_count) : 1u), dim3(64), 0, s, a);   // also clears d_nslow + zero[]
    f = a;
    if (!a.n) return hipGetLastError();
    scan.count = a.wcount;
    scan.row_off = a.wcount;   // in place: tile counts -> block-local tile offsets
    scan.n = ntiles;
    const hipError_t e = launch_scan(scan, s, d_nwords);
    f.bsums = scan.block_sums;
    return e;
}

hipError_t launch_tokenize(const TokArgs& a, ScanArgs scan, uint32_t* d_nwords, hipStream_t s) {
    static const uint32_t cap_fill = resident_blocks(tm_tok_fill, 64);
    TokArgs f;
    const hipError_t e = launch_tok_count_scan(a, scan, d_nwords, s, f);
    if (e != hipSuccess || !a.n) return e != hipSuccess ? e : hipGetLastError();
    const uint32_t ntiles = (a.n + a.tile_topics - 1) / a.tile_topics;
    hipLaunchKernelGGL(tm_tok_fill, dim3(min(ntiles, cap_fill)), dim3(64), 0, s, f);
    return hipGetLastError();
}

hipError_t launch_scatter_keys(DictKey* keys, const uint32_t* idx, const DictKey* vals, uint32_t n, hipStream_t s) {
    if (n) hipLaunchKernelGGL(tm_scatter_keys, dim3((n + 255) / 256), dim3(256), 0, s, keys, idx, vals, n);
    return hipGetLastError();
}

}  // namespace etm
