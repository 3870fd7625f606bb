// cfk_trim.hip — entries leaving the device-resident CommandsForKeys: Pruning.maybePrune (run_cfk_prune)
// and RedundantBefore truncation (run_cfk_truncate). Both mark entries, compact the per-entry arrays
// (compact_entries), derive the snapshot arrays again (cfk_derive) and rebuild the missing() lists
// (rebuild_missing_lists); those steps and the work area are cfk_update.hip's (cfk_work.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cfk_work.hpp"
#include "kernels.hpp"
#include "wave.hpp"

namespace adx {

// =============================================================================================
// Pruning.maybePrune (Pruning.java:164-199) and pruneBefore (:205-331) for a list of keys, on the
// device state. The store's TxnInfo.missing() lists are NO_TXNIDS in this model (the caller checks
// none are loaded), so pruneBefore removes, below the new prunedBefore's byId position, every
// INVALID_OR_TRUNCATED entry and every APPLIED entry executing before it; nothing else moves.
// =============================================================================================
namespace {

// Timestamp.hlc() of dictionary rank r (Timestamp.java:129-131: highHlc(msb) | lowHlc(lsb); the
// normalised lo holds lowHlc << 4)
__device__ __forceinline__ int64_t rank_hlc(const DevSnapshot& s, uint32_t r)
{
    const uint64_t i = (r - 1) >> 1;
    return (int64_t)(((s.dict_hi[i] & 0x7FFFull) << 48) | (s.dict_lo[i] >> 4));
}

__global__ void k_prune_cflag(uint64_t ne, const uint8_t* status, uint32_t* f)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    f[e] = (status[e] >= AD_ST_COMMITTED && status[e] <= AD_ST_APPLIED) ? 1u : 0u;
}

// thread per listed key: the new prunedBefore (maybePrune :166-189) -> p_pos[k] = its byId position
// (0: no prune), p_xr / p_tr = its executeAt / txnId ranks. cm: the committed entries sorted by
// (key, executeAt) (committedByExecuteAt of every key, :651-672); cpos: committed entries before e.
__global__ void k_prune_key(uint64_t nl, const uint32_t* klist, DevSnapshot s, CfkDevState d, const uint32_t* cm,
                            const uint64_t* cpos, int32_t prune_interval, int64_t min_hlc_delta, uint32_t* p_pos,
                            uint32_t* p_xr, uint32_t* p_tr)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nl) return;
    const uint32_t k = klist ? klist[t] : (uint32_t)t;
    const KeyRec kr = d.krec[k];
    if (kr.maw < 0) return;                                   // no APPLIED Write: maxAppliedWrite = -1
    const uint64_t c_lo = cpos[kr.seg_lo], c_hi = cpos[kr.seg_hi];
    // maxAppliedWriteByExecuteAt as an index into the key's committedByExecuteAt
    const uint32_t mx = s.w[kr.maw].x;
    uint64_t lo = c_lo, hi = c_hi;
    while (lo < hi)
    {
        const uint64_t mid = (lo + hi) >> 1;
        if (d.xrank[cm[mid]] < mx) lo = mid + 1;
        else hi = mid;
    }
    const int64_t maw = (int64_t)(lo - c_lo);
    if (maw < (int64_t)prune_interval) return;
    const int64_t max_prune_hlc = rank_hlc(s, mx) - min_hlc_delta;
    int64_t i = maw;
    uint32_t e = 0;
    while (--i >= 0)
    {
        e = cm[c_lo + (uint64_t)i];
        const uint32_t kind = d.ent[e].y >> RANK_BITS;
        if (kind == AD_KIND_WRITE && rank_hlc(s, d.xrank[e]) <= max_prune_hlc && d.status[e] == AD_ST_APPLIED) break;
    }
    if (i < 0) return;
    const uint32_t tr = d.ent[e].y & RANK_MASK;
    if (kr.pruned && tr <= kr.pruned) return;                 // newPrunedBefore <= prunedBefore (:184)
    const uint32_t pos = e - kr.seg_lo;                       // insertPos: it is in byId
    if (pos == 0) return;
    p_pos[k] = pos;
    p_xr[k] = d.xrank[e];
    p_tr[k] = tr;
}

// thread per entry: removed by pruneBefore (:222-254). With missing() lists on the device (d.mref)
// the APPLIED entries are k_prune_subset's to decide; INVALID ones always go.
__global__ void k_prune_mark(uint64_t ne, CfkDevState d, const uint32_t* p_pos, const uint32_t* p_xr, uint32_t* rm)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const uint32_t k = d.ekey[e];
    const uint32_t pos = p_pos[k];
    bool r = false;
    if (pos && e - d.krec[k].seg_lo < pos)
    {
        const uint32_t st = d.status[e];
        r = st == AD_ST_INVALID_OR_TRUNCATED_OR_UNMANAGED_COMMITTED || (!d.mref && st == AD_ST_APPLIED && d.xrank[e] < p_xr[k]);
    }
    rm[e] = r ? 1u : 0u;
}

// thread per pruned key, with missing() lists (:222-251): walking byId below the new prunedBefore,
// an APPLIED entry executing before it goes when its missing() is empty or inside the merged set --
// the new prunedBefore's list united with the lists of the APPLIED entries kept before it that
// execute at their txnId (the set is not built: the kept entries' indices go to `sc`, each id is
// searched in their lists).
__device__ inline bool list_has(const uint64_t* off, const uint32_t* ids, uint32_t L, uint32_t r)
{
    if (L == MREF_NONE || L == MREF_BORN) return false;
    uint64_t lo = off[L], hi = off[L + 1];
    while (lo < hi)
    {
        const uint64_t m = (lo + hi) >> 1;
        if (ids[m] < r) lo = m + 1;
        else hi = m;
    }
    return lo < off[L + 1] && ids[lo] == r;
}

__global__ void k_prune_subset(uint64_t nl, const uint32_t* klist, CfkDevState d, const uint32_t* p_pos, const uint32_t* p_xr,
                               const uint64_t* moff, const uint32_t* mids, uint32_t* sc, uint32_t* rm)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nl) return;
    const uint32_t k = klist ? klist[t] : (uint32_t)t;
    const uint32_t pos = p_pos[k];
    if (!pos) return;
    const uint32_t lo = d.krec[k].seg_lo, npb = lo + pos, x_npb = p_xr[k];
    const uint32_t L0 = d.mref[npb];
    uint32_t nret = 0;
    for (uint32_t e = lo; e < npb; ++e)
    {
        if (d.status[e] != AD_ST_APPLIED || d.xrank[e] >= x_npb) continue;
        const uint32_t L = d.mref[e];
        bool subset = true;
        if (L != MREF_NONE && L != MREF_BORN)
            for (uint64_t j = moff[L]; j < moff[L + 1] && subset; ++j)
            {
                const uint32_t r = mids[j];
                bool in = list_has(moff, mids, L0, r);
                for (uint32_t q = 0; q < nret && !in; ++q) in = list_has(moff, mids, d.mref[sc[lo + q]], r);
                subset = in;
            }
        if (subset)
        {
            rm[e] = 1u;
            continue;
        }
        if (d.xrank[e] == (d.ent[e].y & RANK_MASK)) sc[lo + nret++] = e;
    }
}

// thread per key: segments after the removals; prunedBefore where entries went (:255-257: a key
// without removals keeps its CommandsForKey, prunedBefore included)
__global__ void k_prune_keys(uint64_t nk, KeyRec* krec, const uint64_t* rpos, const uint32_t* p_pos, const uint32_t* p_tr,
                             unsigned long long* n_keys_pruned)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nk) return;
    KeyRec kr = krec[k];
    const uint64_t r_lo = rpos[kr.seg_lo], r_hi = rpos[kr.seg_hi];
    if (p_pos[k] && r_hi > r_lo)
    {
        kr.pruned = p_tr[k];
        atomicAdd(n_keys_pruned, 1ull);
    }
    kr.seg_lo -= (uint32_t)r_lo;
    kr.seg_hi -= (uint32_t)r_hi;
    krec[k] = kr;
}

}  // namespace

int run_cfk_prune(CfkStore& cs, const uint32_t* klist, uint64_t nl, int32_t prune_interval, int64_t min_hlc_delta,
                  CfkPruneOut* out)
{
    CfkUpdWork* w = cs.w;
    DevSnapshot& s = cs.s;
    CfkDevState& d = cs.d;
    const hipStream_t st = cs.st;
    *out = CfkPruneOut{};
    const uint64_t ne = s.n_ent, nk = s.n_keys;
    if (!nk || !ne || !nl) return AD_OK;
    if (int rc = cfk_begin(cs)) return rc;
    UpdCtl* ctl = w->ctl.as<UpdCtl>();
    // the committed order of the current entries (a derivation keeps it; after the ingest, derive once)
    if (!w->cm_valid)
    {
        UALLOC(w->chg[w->chg_cur], ne, false);
        w->moved = false;
        if (int rc = cfk_derive(cs)) return rc;
        UCHK(hipMemsetAsync(ctl, 0, sizeof(UpdCtl), st));
    }
    UALLOC(w->flags, 4 * ne, false);
    UALLOC(w->fs, 8 * (ne + 1), false);
    UALLOC(w->bsum, 8 * ((ne + 1023) / 1024 + 8), false);
    UALLOC(w->maw, 4 * nk, false);          // p_pos
    UALLOC(w->wtail, 4 * nk, false);        // p_xr
    UALLOC(w->gkey, 4 * nk, false);         // p_tr
    UALLOC(w->uflag, 4 * ne, false);        // rm
    UALLOC(w->upos, 8 * (ne + 1), false);   // rpos
    uint32_t* p_pos = w->maw.as<uint32_t>();
    uint32_t* p_xr = w->wtail.as<uint32_t>();
    uint32_t* p_tr = w->gkey.as<uint32_t>();
    k_prune_cflag<<<blocks(ne), 256, 0, st>>>(ne, d.status, w->flags.as<uint32_t>());
    UCHK(run_scan_arrays(w->flags.as<uint32_t>(), w->fs.as<uint64_t>(), ne, 1, w->bsum.as<uint64_t>(), st));
    UCHK(hipMemsetAsync(p_pos, 0, 4 * nk, st));
    k_prune_key<<<blocks(nl), 256, 0, st>>>(nl, klist, s, d, w->cm.as<uint32_t>(), w->fs.as<uint64_t>(), prune_interval,
                                            min_hlc_delta, p_pos, p_xr, p_tr);
    k_prune_mark<<<blocks(ne), 256, 0, st>>>(ne, d, p_pos, p_xr, w->uflag.as<uint32_t>());
    const bool lists = d.mref && cs.miss.on;
    if (lists)
    {
        UALLOC(w->dsrc, 4 * ne, false);       // the subset walk's kept entries (per key, in its segment)
        k_prune_subset<<<blocks(nl), 256, 0, st>>>(nl, klist, d, p_pos, p_xr, cs.miss.off, cs.miss.ids, w->dsrc.as<uint32_t>(),
                                                   w->uflag.as<uint32_t>());
    }
    UCHK(hipGetLastError());
    if (int rc = scan_removed(cs, ne)) return rc;
    UCHK(d2h(w->h_ctl, ctl, sizeof(UpdCtl), st));
    UCHK(hipStreamSynchronize(st));
    const uint64_t R = w->h_ctl->tot2[0];
    if (R == 0) return cfk_elapsed(cs, &out->ms_total);
    // compaction into the spare per-entry arrays, segments and prunedBefore, then a full derivation
    unsigned long long* nkp = reinterpret_cast<unsigned long long*>(&ctl->tot2[1]);
    UCHK(hipMemsetAsync(nkp, 0, 8, st));
    if (int rc = compact_entries(cs, w->uflag.as<uint32_t>(), w->upos.as<uint64_t>(), R, [&] {
            k_prune_keys<<<blocks(nk), 256, 0, st>>>(nk, d.krec, w->upos.as<uint64_t>(), p_pos, p_tr, nkp);
        }))
        return rc;
    UCHK(d2h(w->h_ctl, ctl, sizeof(UpdCtl), st));
    UCHK(hipStreamSynchronize(st));
    out->n_keys_pruned = w->h_ctl->tot2[1];
    out->n_removed = R;
    UCHK(hipMemsetAsync(ctl, 0, sizeof(UpdCtl), st));
    if (int rc = cfk_derive(cs)) return rc;
    if (lists)
    {
        // the kept entries' lists, compacted again (each entry its own list, pruned ones dropped)
        UALLOC(w->dsrc, 4 * s.n_ent, false);
        UCHK(hipMemsetAsync(w->dsrc.p, 0xFF, 4 * s.n_ent, st));
        if (int rc = rebuild_missing_from_entries(cs, CfkUpdIn{}, nullptr)) return rc;
    }
    if (int rc = cfk_elapsed(cs, &out->ms_total)) return rc;
    UCHK(d2h(w->h_ctl, ctl, sizeof(UpdCtl), st));
    UCHK(hipStreamSynchronize(st));
    if (w->h_ctl->err) { cs.err = "derivation after pruning reported an inconsistency"; return AD_E_STATE; }
    return AD_OK;
}

// =============================================================================================
// RedundantBefore on the device: SafeCommandStore.maybeTruncate (SafeCommandStore.java:165-171) ->
// SafeCommandsForKey.updateRedundantBefore -> CommandsForKey.withRedundantBeforeAtLeast
// (CommandsForKey.java:1317-1341). For every key, the byId entries below its RedundantBefore entry's
// shardRedundantBefore leave and the missing() lists of the rest lose the ids below it
// (Utils.removeRedundantMissing, Utils.java:265-275) -- both only where something left
// (insertPos != 0); a prunedBefore at or below it becomes NO_INFO (the constructor, :646-648). The
// watermarks are the snapshot's rb_wm ranks (dictionary members; 0 = NONE).
// =============================================================================================
namespace {

// the RedundantBefore entry holding key x (RedundantBefore.get: a lookup over the disjoint ascending
// entries; epochs not read), or ~0
__device__ inline uint64_t rb_entry_holding(const DevSnapshot& s, int64_t x)
{
    const bool incl = s.start_inclusive != 0;
    uint64_t lo = 0, hi = s.n_rb;
    while (lo < hi)
    {
        const uint64_t m = (lo + hi) >> 1;
        if (incl ? s.rb_start[m] <= x : s.rb_start[m] < x) lo = m + 1;
        else hi = m;
    }
    if (!lo) return ~0ull;
    return range_contains(s.start_inclusive, s.rb_start[lo - 1], s.rb_end[lo - 1], x) ? lo - 1 : ~0ull;
}

// thread per key: t_pos[k] = insertPos(shardRedundantBefore) within byId (the entries that leave),
// t_wm[k] = its rank (0: NONE or no entry); a prunedBefore at or below it is cleared in place;
// *n_chg counts the keys that change
__global__ void k_trunc_key(uint64_t nk, DevSnapshot s, KeyRec* krec, uint32_t* t_pos, uint32_t* t_wm,
                            unsigned long long* n_chg)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nk) return;
    uint32_t pos = 0, wm = 0;
    const uint64_t e = rb_entry_holding(s, s.keys[k]);
    if (e != ~0ull) wm = s.rb_wm[e];
    bool chg = false;
    if (wm)
    {
        const KeyRec kr = krec[k];
        uint32_t lo = kr.seg_lo, hi = kr.seg_hi;
        while (lo < hi)
        {
            const uint32_t m = (lo + hi) >> 1;
            if ((s.ent[m].y & RANK_MASK) < wm) lo = m + 1;
            else hi = m;
        }
        pos = lo - kr.seg_lo;
        chg = pos != 0;
        if (kr.pruned && wm >= kr.pruned)
        {
            krec[k].pruned = 0;
            chg = true;
        }
    }
    t_pos[k] = pos;
    t_wm[k] = wm;
    if (chg) atomicAdd(n_chg, 1ull);
}

// byId segments from this length are searched by their wave (64 pivots a round, wave_lower_bound); shorter ones
// by their own lane (at most 7 dependent loads). The wave takes its long keys one after the other, about two
// dependent rounds each, so it pays only while they are few: above TRUNC_COOP_MAX long keys in a wave every lane
// searches its own segment (log2 of the longest, in parallel). Both constants are reasoned, not measured.
constexpr uint32_t TRUNC_COOP_MIN = 128;
constexpr uint32_t TRUNC_COOP_MAX = 4;

// k_trunc_key for the keys inside the risen spans only (ad_redundant_merge). The key array is ascending (ingest
// checks it, new keys are merged in place), so a span holds one run of key ordinals [k0, k1): blockIdx.y walks the
// spans, the blocks of a row stride over the span's run, lane per key. Every block of a row finds the run with
// the same two searches (uniform loads, 2 * log2(nk) steps) -- no bounds pass and no read-back in between.
// Sized for what a RedundantBefore.create step yields, one to a few spans (one per sub-range, more only when the
// addition crosses entries of other watermarks): the repeated searches and the up to 64 blocks a row are noise
// then. Thousands of tiny spans would still be correct (rows stride from 1024 spans on) but would want a bounds
// pass and one flat grid instead.
// t_pos / t_wm were cleared: the keys outside the spans keep 0. *n_exam counts the keys inside.
__global__ __launch_bounds__(256) void k_trunc_spans(uint64_t nk, DevSnapshot s, const RbSpan* spans, uint64_t n_spans,
                                                     KeyRec* krec, uint32_t* t_pos, uint32_t* t_wm,
                                                     unsigned long long* n_chg, unsigned long long* n_exam)
{
    const uint32_t lane = lane_id();
    const bool incl = s.start_inclusive != 0;
    for (uint64_t sp = blockIdx.y; sp < n_spans; sp += gridDim.y)
    {
        const RbSpan span = spans[sp];
        // keys before bound b's side of a range: key < b (StartInclusive), key <= b (EndInclusive)
        auto ordinal = [&](int64_t b) -> uint64_t {
            uint64_t lo = 0, hi = nk;
            while (lo < hi)
            {
                const uint64_t m = (lo + hi) >> 1;
                const int64_t x = s.keys[m];
                if (incl ? x < b : x <= b) lo = m + 1;
                else hi = m;
            }
            return lo;
        };
        const uint64_t k0 = ordinal(span.start), k1 = ordinal(span.end);
        const uint64_t cnt = k1 > k0 ? k1 - k0 : 0;
        if (blockIdx.x == 0 && threadIdx.x == 0 && cnt) atomicAdd(n_exam, (unsigned long long)cnt);
        // block-uniform trip count: every lane of a wave reaches the ballots below
        for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < cnt; base += (uint64_t)gridDim.x * blockDim.x)
        {
            const uint64_t i = base + threadIdx.x;
            const bool on = i < cnt;
            const uint64_t k = k0 + (on ? i : 0);
            const KeyRec kr = krec[k];
            uint32_t lo = kr.seg_lo, hi = kr.seg_hi;
            const bool lng = on && hi - lo >= TRUNC_COOP_MIN;
            const uint32_t n_lng = (uint32_t)__popcll(ballot(lng));
            const bool coop = lng && n_lng <= TRUNC_COOP_MAX;
            if (on && !coop)
                while (lo < hi)
                {
                    const uint32_t m = (lo + hi) >> 1;
                    if ((s.ent[m].y & RANK_MASK) < span.wm) lo = m + 1;
                    else hi = m;
                }
            // long segments, one at a time by the whole wave
            uint64_t todo = ballot(coop);
            while (todo)
            {
                const int src = __ffsll((unsigned long long)todo) - 1;
                todo &= todo - 1;
                const uint32_t a = (uint32_t)__shfl((int)lo, src, 64), b = (uint32_t)__shfl((int)hi, src, 64);
                const uint32_t p = (uint32_t)wave_lower_bound(
                    a, b, [&](uint64_t x) { return s.ent[x].y & RANK_MASK; }, [&](uint32_t r) { return r < span.wm; });
                if ((int)lane == src) lo = p;
            }
            const uint32_t pos = lo - kr.seg_lo;
            bool chg = on && pos != 0;
            if (on && kr.pruned && span.wm >= kr.pruned)
            {
                krec[k].pruned = 0;
                chg = true;
            }
            if (on)
            {
                t_pos[k] = pos;
                t_wm[k] = span.wm;
            }
            const uint32_t nc = (uint32_t)__popcll(ballot(chg));
            if (lane == 0 && nc) atomicAdd(n_chg, (unsigned long long)nc);
        }
    }
}

// thread per entry: below its key's shardRedundantBefore (a prefix of the key's byId)
__global__ void k_trunc_mark(uint64_t ne, const uint32_t* ekey, const KeyRec* krec, const uint32_t* t_pos, uint32_t* rm)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ne) return;
    const uint32_t k = ekey[e];
    rm[e] = (e - krec[k].seg_lo < t_pos[k]) ? 1u : 0u;
}

// thread per key: segments after the removals (an emptied byId has no last txnId)
__global__ void k_trunc_keys(uint64_t nk, KeyRec* krec, const uint64_t* rpos)
{
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nk) return;
    KeyRec kr = krec[k];
    kr.seg_lo -= (uint32_t)rpos[kr.seg_lo];
    kr.seg_hi -= (uint32_t)rpos[kr.seg_hi];
    if (kr.seg_hi == kr.seg_lo) kr.last_txn = 0;
    krec[k] = kr;
}

// thread per kept entry (its list mref[j] of the old CSR): the ids at or above the key's
// shardRedundantBefore where entries left (removeRedundantMissing), all of them elsewhere. Pass 0
// counts, pass 1 writes.
template <int WRITE>
__global__ __launch_bounds__(256) void k_trunc_miss(uint64_t n, const uint32_t* mref, const uint32_t* ekey,
                                                    const uint32_t* t_pos, const uint32_t* t_wm, const uint64_t* ooff,
                                                    const uint32_t* oids, uint32_t* cnt, const uint64_t* noff, uint32_t* nids)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t L = mref[j];
    uint64_t c = 0, o = WRITE ? noff[j] : 0;
    if (L != MREF_NONE && L != MREF_BORN)
    {
        const uint32_t k = ekey[j];
        const uint32_t lb = t_pos[k] ? t_wm[k] : 0;
        for (uint64_t a = ooff[L]; a < ooff[L + 1]; ++a)
        {
            const uint32_t r = oids[a];
            if (r < lb) continue;
            if (WRITE) nids[o++] = r;
            ++c;
        }
    }
    if (!WRITE) cnt[j] = (uint32_t)c;
}

}  // namespace

int run_cfk_truncate(CfkStore& cs, uint32_t* h_pos, const RbSpan* spans, uint64_t n_spans, CfkTruncOut* out)
{
    CfkUpdWork* w = cs.w;
    DevSnapshot& s = cs.s;
    CfkDevState& d = cs.d;
    const hipStream_t st = cs.st;
    *out = CfkTruncOut{};
    const uint64_t ne = s.n_ent, nk = s.n_keys;
    if (!nk || !s.n_rb || (spans && !n_spans)) return AD_OK;
    if (int rc = cfk_begin(cs)) return rc;
    UpdCtl* ctl = w->ctl.as<UpdCtl>();
    UALLOC(w->tpos, 4 * nk, false);
    UALLOC(w->twm, 4 * nk, false);
    uint32_t* t_pos = w->tpos.as<uint32_t>();
    uint32_t* t_wm = w->twm.as<uint32_t>();
    unsigned long long* n_chg = reinterpret_cast<unsigned long long*>(&ctl->tot2[1]);
    if (spans)
    {
        // the keys outside the spans keep t_pos = t_wm = 0; a row of blocks per span (rows and blocks stride)
        UCHK(hipMemsetAsync(t_pos, 0, 4 * nk, st));
        UCHK(hipMemsetAsync(t_wm, 0, 4 * nk, st));
        const dim3 grid(std::min(blocks(nk), 64u), (unsigned)std::min<uint64_t>(n_spans, 1024));
        k_trunc_spans<<<grid, 256, 0, st>>>(nk, s, spans, n_spans, d.krec, t_pos, t_wm, n_chg,
                                            reinterpret_cast<unsigned long long*>(&ctl->tot3[0]));
    }
    else
        k_trunc_key<<<blocks(nk), 256, 0, st>>>(nk, s, d.krec, t_pos, t_wm, n_chg);
    if (ne)
    {
        UALLOC(w->uflag, 4 * ne, false);        // rm
        UALLOC(w->upos, 8 * (ne + 1), false);   // rpos
        k_trunc_mark<<<blocks(ne), 256, 0, st>>>(ne, d.ekey, d.krec, t_pos, w->uflag.as<uint32_t>());
        if (int rc = scan_removed(cs, ne)) return rc;
    }
    UCHK(hipGetLastError());
    UCHK(d2h(w->h_ctl, ctl, sizeof(UpdCtl), st));
    UCHK(hipStreamSynchronize(st));
    const uint64_t R = ne ? w->h_ctl->tot2[0] : 0, changed = w->h_ctl->tot2[1];
    out->n_examined = spans ? w->h_ctl->tot3[0] : nk;
    if (!changed) return cfk_elapsed(cs, &out->ms_total);
    if (h_pos) UCHK(d2h(h_pos, t_pos, 4 * nk, st));      // the host's lists follow (the caller trims them)
    if (!R)
    {
        // only prunedBefore moved (krec, in place): nothing derived reads it
        out->n_keys = changed;
        return cfk_elapsed(cs, &out->ms_total);
    }
    // compaction into the spare per-entry arrays and the segments, as pruning does
    if (int rc = compact_entries(cs, w->uflag.as<uint32_t>(), w->upos.as<uint64_t>(), R,
                                 [&] { k_trunc_keys<<<blocks(nk), 256, 0, st>>>(nk, d.krec, w->upos.as<uint64_t>()); }))
        return rc;
    UCHK(hipMemsetAsync(ctl, 0, sizeof(UpdCtl), st));
    if (int rc = cfk_derive(cs)) return rc;
    if (d.mref && cs.miss.on)
    {
        // the kept entries' lists, trimmed and compacted (each entry its own list again)
        const uint64_t n2 = s.n_ent;
        if (int rc = rebuild_missing_lists(
                cs, n2,
                [&](uint32_t* cnt) {
                    k_trunc_miss<0><<<blocks(n2), 256, 0, st>>>(n2, d.mref, d.ekey, t_pos, t_wm, cs.miss.off, cs.miss.ids, cnt,
                                                                nullptr, nullptr);
                },
                [&](const uint64_t* noff, uint32_t* nids) {
                    k_trunc_miss<1><<<blocks(n2), 256, 0, st>>>(n2, d.mref, d.ekey, t_pos, t_wm, cs.miss.off, cs.miss.ids, nullptr,
                                                                noff, nids);
                }))
            return rc;
    }
    UCHK(d2h(w->h_ctl, ctl, sizeof(UpdCtl), st));
    UCHK(hipStreamSynchronize(st));
    if (w->h_ctl->err) { cs.err = "derivation after truncation reported an inconsistency"; return AD_E_STATE; }
    out->n_removed = R;
    out->n_keys = changed;
    return cfk_elapsed(cs, &out->ms_total);
}

}  // namespace adx
