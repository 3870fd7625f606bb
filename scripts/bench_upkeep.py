#!/usr/bin/env python3
"""Store upkeep cost on a config-2 store: a RedundantBefore advance in place
(ad_redundant_advance: watermark dictionary growth + device truncation) against the rebuild a full
ad_redundant_load costs (the whole snapshot rebuilt from the host copies, then truncated).

  python scripts/bench_upkeep.py [--hist 16000000 --keys 1000000 --txns 200000 --advances 4]
  python scripts/bench_upkeep.py --merge --entries 16      ad_redundant_merge of a sub-range (boundary change)

Prints one JSON line per measurement and a summary line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cassandra-accord_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from accord_deps import native, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hist", type=int, default=16_000_000)
    ap.add_argument("--keys", type=int, default=1_000_000)
    ap.add_argument("--txns", type=int, default=200_000)
    ap.add_argument("--entries", type=int, default=64, help="RedundantBefore entries")
    ap.add_argument("--advances", type=int, default=4)
    ap.add_argument("--registry", action="store_true", help="range-command registry upkeep on config 4 instead")
    ap.add_argument("--rows", type=int, default=1000, help="registry rows per upkeep batch")
    ap.add_argument("--merge", action="store_true", help="ad_redundant_merge of a sub-range (use --entries 16) instead")
    a = ap.parse_args()
    if a.registry:
        return registry(a)
    if a.merge:
        return merge(a)
    t0 = time.time()
    w = synth.with_redundant_ranges(synth.config2(n_txns=a.txns, n_keys=a.keys, n_hist_entries=a.hist), a.entries,
                                    seed=5, wm_frac=0.2)
    print("# workload %.1fs: %d entries, %d RedundantBefore entries" % (time.time() - t0, w.cfk.n_entries,
                                                                        len(w.redundant.range_start)), flush=True)
    hist = int(synth._hlc(w.cfk.txn).max())
    st = native.DeviceCommandStore(0)
    L = native.lib()
    try:
        t = time.time()
        st.load(w)
        load_ms = (time.time() - t) * 1e3
        print(json.dumps(dict(what="load+prepare", ms=round(load_ms, 2))), flush=True)
        red = w.redundant
        adv, reb = [], []
        for i in range(a.advances):
            red = synth.advance_redundant(red, 100 + i, step_frac=0.03, hist_hlc=hist)
            t = time.time()
            s = st.redundant_advance(red)
            ms = (time.time() - t) * 1e3
            adv.append(ms)
            print(json.dumps(dict(what="advance", step=i, ms=round(ms, 2), ms_device=round(s["ms_device"], 3),
                                  ms_dict=round(s["ms_stage"][0], 3), removed=int(s["n_keys"][0]),
                                  keys_changed=int(s["n_keys"][1]), new_ids=int(s["n_keys"][2]))), flush=True)
            # the same state through the full-replacement route: ad_redundant_load + the rebuild it forces
            t = time.time()
            st._check(L.ad_redundant_load(st.h, C.byref(red.soa())))
            st._check(L.ad_prepare(st.h))
            ms = (time.time() - t) * 1e3
            reb.append(ms)
            print(json.dumps(dict(what="redundant_load+rebuild", step=i, ms=round(ms, 2))), flush=True)
        print(json.dumps(dict(metric="redundant_before_upkeep", entries=int(w.cfk.n_entries),
                              advance_ms_median=round(sorted(adv)[len(adv) // 2], 2),
                              rebuild_ms_median=round(sorted(reb)[len(reb) // 2], 2))), flush=True)
    finally:
        st.close()


def merge(a):
    """ad_redundant_merge on the config-2 store: each step advances about 1/32 of the key line inside the widest
    entry (step 0 splits it, later steps move the same piece: watermarks only), against the two older routes to the
    same state on stores loaded alike -- ad_redundant_load + the rebuild it forces (the only one for a boundary
    change), and ad_redundant_advance of the whole enclosing entry to the same watermark (more keys examined,
    and a larger watermark move than asked for)."""
    from accord_deps.model import Redundant
    t0 = time.time()
    w = synth.with_redundant_ranges(synth.config2(n_txns=a.txns, n_keys=a.keys, n_hist_entries=a.hist), a.entries,
                                    seed=5, wm_frac=0.2)
    hist = int(synth._hlc(w.cfk.txn).max())
    keys = w.cfk.keys
    print("# workload %.1fs: %d entries, %d keys, %d RedundantBefore entries" % (
        time.time() - t0, w.cfk.n_entries, len(keys), len(w.redundant.range_start)), flush=True)
    red0 = w.redundant
    order = (red0.range_end - red0.range_start).argsort()[::-1].tolist()      # entries, widest first
    big = int(order[0])

    def piece_of(i, share):
        """the middle `share` keys of entry i as a range"""
        ks = keys[(keys > red0.range_start[i]) & (keys < red0.range_end[i])]
        assert len(ks) > share + 2, "entry %d holds too few keys" % i
        return (int(ks[len(ks) // 2 - share // 2]), int(ks[len(ks) // 2 + share // 2]))

    piece = piece_of(big, max(2, len(keys) // 32))
    sm, sa, sr = (native.DeviceCommandStore(0) for _ in range(3))
    L = native.lib()

    def rebuild(red):
        t = time.time()
        sr._check(L.ad_redundant_load(sr.h, C.byref(red.soa())))
        sr._check(L.ad_prepare(sr.h))
        return (time.time() - t) * 1e3

    def show(what, step, ms, s, **kw):
        print(json.dumps(dict(what=what, step=step, ms=round(ms, 2), ms_device=round(s["ms_device"], 3),
                              ms_dict=round(s["ms_stage"][0], 3), ms_refresh=round(s["ms_stage"][1], 3),
                              n_probes=int(s["n_probes"]), removed=int(s["n_keys"][0]), keys_changed=int(s["n_keys"][1]),
                              new_ids=int(s["n_keys"][2]), **kw)), flush=True)

    try:
        for st in (sm, sa, sr):
            st.load(w)
        # warm-up, discarded: a split and a watermark move in another entry on every store -- the first-time
        # dictionary merge, the work buffers and the span buffer are then in place for the measured steps
        red = red0
        for i in range(2):
            red = synth.merge_redundant(red, 290 + i, ranges=[piece_of(int(order[4]), 64)], hist_hlc=hist, step_frac=0.03)
            sm.redundant_merge(red)
        sa.redundant_merge(red)
        rebuild(red)
        whole = red
        mer, adv, reb, spl = [], [], [], []
        for i in range(a.advances):
            red, add = synth.merge_redundant(red, 300 + i, ranges=[piece], hist_hlc=hist, step_frac=0.03, return_add=True)
            t = time.time()
            s = sm.redundant_merge(red)
            ms = (time.time() - t) * 1e3
            mer.append(ms)
            show("merge", i, ms, s, boundaries_changed=(i == 0))
            # the whole enclosing entry moved to the same watermark with the old call
            j = int(((whole.range_start <= piece[0]) & (whole.range_end >= piece[1])).argmax())
            wm = whole.wm.take(list(range(len(whole.range_start))))
            wm.msb[j], wm.lsb[j], wm.node[j] = add.wm.msb[0], add.wm.lsb[0], add.wm.node[0]
            whole = Redundant(whole.range_start, whole.range_end, whole.start_epoch, whole.end_epoch, wm)
            t = time.time()
            s = sa.redundant_advance(whole)
            ms = (time.time() - t) * 1e3
            adv.append(ms)
            show("advance_whole_entry", i, ms, s)
            ms = rebuild(red)
            reb.append(ms)
            print(json.dumps(dict(what="redundant_load+rebuild", step=i, ms=round(ms, 2))), flush=True)
        # the boundary change again, on fresh pieces of other entries: more samples of a split
        for n, i in enumerate(order[1:4]):
            red = synth.merge_redundant(red, 400 + n, ranges=[piece_of(int(i), max(2, len(keys) // 64))], hist_hlc=hist,
                                        step_frac=0.03)
            t = time.time()
            s = sm.redundant_merge(red)
            ms = (time.time() - t) * 1e3
            spl.append(ms)
            show("merge_split_again", n, ms, s, boundaries_changed=True)
        med = lambda v: round(sorted(v)[len(v) // 2], 2)  # noqa: E731
        print(json.dumps(dict(metric="redundant_before_merge", entries=int(w.cfk.n_entries), keys=int(len(keys)),
                              merge_split_ms=round(mer[0], 2), merge_split_again_ms_median=med(spl),
                              merge_wm_only_ms_median=med(mer[1:] or mer), advance_ms_median=med(adv),
                              rebuild_ms_median=med(reb))), flush=True)
    finally:
        for st in (sm, sa, sr):
            st.close()


def registry(a):
    """config 4 (100k range commands over 1M keys): ad_range_cmds_update batches of `rows` registrations / unions /
    erasures / historical merges against the ad_range_cmds_load (full rebuild) of the same registry."""
    import refmodel
    t0 = time.time()
    w = synth.config4()
    lo, hi = int(w.cfk.keys.min()), int(w.cfk.keys.max())
    print("# config4 %.1fs: %d entries, %d range commands" % (time.time() - t0, w.cfk.n_entries, len(w.cmds.txn.msb)),
          flush=True)
    st = native.DeviceCommandStore(0)
    L = native.lib()
    try:
        st.load(w)
        cmds = w.cmds
        upd, reb = [], []
        for i in range(a.advances):
            u = synth.range_cmd_updates(cmds, 200 + i, a.rows, lo=lo, hi=hi, hlc_hi=90000, max_width=(hi - lo) // 20000)
            t = time.time()
            s = st.range_cmds_update(u)
            ms = (time.time() - t) * 1e3
            upd.append(ms)
            cmds = refmodel.range_cmds_update(cmds, u)
            print(json.dumps(dict(what="range_cmds_update", step=i, ms=round(ms, 2), ms_host=round(s["ms_stage"][0], 2),
                                  ms_refresh=round(s["ms_stage"][1], 2), registered=int(s["n_keys"][0]),
                                  range_entries=int(s["n_keys"][1]), new_ids=int(s["n_keys"][2]))), flush=True)
            t = time.time()
            st._check(L.ad_range_cmds_load(st.h, C.byref(cmds.soa())))
            st._check(L.ad_prepare(st.h))
            ms = (time.time() - t) * 1e3
            reb.append(ms)
            print(json.dumps(dict(what="range_cmds_load+rebuild", step=i, ms=round(ms, 2))), flush=True)
        print(json.dumps(dict(metric="range_registry_upkeep", rows=a.rows, commands=int(len(cmds.txn.msb)),
                              update_ms_median=round(sorted(upd)[len(upd) // 2], 2),
                              rebuild_ms_median=round(sorted(reb)[len(reb) // 2], 2))), flush=True)
    finally:
        st.close()


if __name__ == "__main__":
    main()
