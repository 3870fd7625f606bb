// cfk_work.hpp — what cfk_update.hip (update, derivation, dictionary growth) and cfk_trim.hip (pruning,
// RedundantBefore truncation) share: the persistent work area, the control block, and the host steps
// every run_cfk_* call is made of. Internal to those two files.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <functional>
#include <string>

#include "../../include/accord_deps.h"
#include "cfk_update.hpp"
#include "devmem.hpp"

namespace adx {

struct UpdCtl {
    uint32_t err, err_idx;
    unsigned long long applied;
    uint64_t tot[4];          // cand per class, committed entries
    uint64_t tot2[2];         // new dictionary ids (unique), inserted entries (groups)
    uint64_t tot3[2];         // insertion updates, present updates (ballot fold)
    uint32_t n_new, n_ins;    // ids the dictionary does not hold, insertion updates
    unsigned long long diff[3];   // OR of (word ^ reference) over the new ids: node, lo, hi (sort digits)
    uint32_t older, pad;      // a new id is older than the newest dictionary id (dictionary merge)
    uint64_t cm[2];           // incremental committed order: entries kept from the last one, changed committed entries
    uint32_t n_newk, pad2;    // update keys without a CommandsForKey (with repeats)
    unsigned long long kdiff; // OR of (key ^ the batch's first key) over them, sign-flipped (sort digits)
};

struct EntArrays { uint2* ent; uint8_t* status; uint32_t* xrank; uint32_t* ekey; Bal* bal; uint8_t* chg; uint32_t* mref; };

inline unsigned blocks(uint64_t n, unsigned t = 256) { return (unsigned)std::max<uint64_t>(1, (n + t - 1) / t); }

// grows with slack (insertions raise the entry count every batch: no reallocation, and no re-zeroing
// of `word`, per batch); zero: the whole new allocation is zeroed
struct DBuf : DevBuf {
    bool ensure(size_t b, bool zero = false) { return grow(b, zero); }
};

struct CfkUpdWork {
    DBuf ctl, loc, xr, word, bk, flags, fs, bsum, ck, cv, ck2, cv2, hist, hoff, f2, s2, maw, wtail, kmap;
    DBuf sm_hi, sm_lo, sm_node;
    DBuf nw, nk_a, nk_b, nv_a, nv_b, nflag, npos, ins_k, ins_v, gflag, gs, gword, gkey, grank, ib, krec_bk;
    DBuf mh, ml, mn, mraw, mpos;
    DBuf bkb, uflag, upos, rk;
    // missing() maintenance: per update applied flags, dep ranks, additions batch, derivation
    DBuf uapp, drank, acnt, aoff, a_k, a_tm, a_tl, a_tn, a_st, dsrc, mflag, mpp, mpend, mcnt, moff;
    // byId's last txnId as each update sees it (additions past the end) and the LoadPruned ids
    DBuf trk, pk, pv, pk2, pv2, pvv, pw, pe, pbm, plast, ppos, lcnt, loff, l_k, l_tm, l_tl, l_tn, l_i;
    DBuf kn_a, kn_b, kv_a, kv_b, kflag, kfpos, knew, kpos;   // new keys
    DBuf tpos, twm, ids_st, ids_rank;                          // RedundantBefore truncation / dictionary ensure
    // incremental committed order: the last derivation's order (entry indices), per-entry changed
    // flags (double-buffered with the entry arrays), the insertion's old -> new entry map
    DBuf cm, chg[2], mv, af, ap, bfl, bps, cka, cva, ckb, cvb, ckb2, cvb2;
    int chg_cur = 0;
    uint64_t cm_n = 0;
    bool cm_valid = false, moved = false;
    UpdCtl* h_ctl = nullptr;
    hipEvent_t ev[3] = {};
    ~CfkUpdWork()
    {
        if (h_ctl) (void)hipHostFree(h_ctl);
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// both need a CfkStore& cs in scope: the message goes to cs.err
#define UCHK(expr)                                                                                \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) { cs.err = std::string(#expr) + ": " + hipGetErrorString(_e); return AD_E_DEVICE; } \
    } while (0)
#define UALLOC(buf, bytes, zero)                                                                  \
    do {                                                                                          \
        if (!(buf).ensure((bytes), (zero))) { cs.err = "device allocation (cfk update)"; return AD_E_NOMEM; } \
    } while (0)

// ---- the host steps shared by the run_cfk_* calls (cfk_update.hip) ----

// Start of a call: the pinned copy of the control block and the timing events exist, the device control
// block is zeroed and ev[0] recorded on the stream.
int cfk_begin(CfkStore& cs);
// Records and waits for ev[1]: the milliseconds since cfk_begin's ev[0].
int cfk_elapsed(CfkStore& cs, double* ms);

// Rebuild ent.tau, cand, cwr, w, krec, kent and the trees from the per-entry state (status,
// executeAt rank). A duplicate committed executeAt is reported in ctl->err. incr: the committed order
// from the last derivation's, where that still stands.
int cfk_derive(CfkStore& cs, bool incr = false);

// The removal flags w->uflag (one per entry, ne of them) scanned into w->upos (both the caller's), the
// number of flagged entries left in ctl->tot2[0].
int scan_removed(CfkStore& cs, uint64_t ne);

// The entries flagged in rm (rpos: its exclusive scan, R flagged in all, R > 0) leave: the kept ones
// move to the spare per-entry arrays (k_prune_move), per_key launches the caller's kernel that moves the
// key segments, the arrays are swapped and the snapshot's view follows. The committed order is dropped
// (entry indices changed: the next derivation sorts afresh).
int compact_entries(CfkStore& cs, const uint32_t* rm, const uint64_t* rpos, uint64_t R, const std::function<void()>& per_key);

// The missing() CSR built again, one list per entry (n = the entry count): count(cnt) launches the
// kernel that writes list j's length to cnt[j], emit(off, ids) the one that writes its ids from off[j];
// both read the current CSR (cs.miss). Then mref[j] = j and the new CSR is current.
int rebuild_missing_lists(CfkStore& cs, uint64_t n, const std::function<void(uint32_t*)>& count,
                          const std::function<void(const uint64_t*, uint32_t*)>& emit);

// rebuild_missing_lists by k_miss_build: every entry's list from its current one and the entries born
// since (k_miss_flags / k_miss_scatter), or from update u's deps where w->dsrc (the caller's, n_ent
// entries, 0xFFFFFFFF = none) names the update; drank: the deps' ranks (null with no sources).
int rebuild_missing_from_entries(CfkStore& cs, const CfkUpdIn& u, const uint32_t* drank);

}  // namespace adx
