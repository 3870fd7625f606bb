#!/usr/bin/env python3
"""ad_deps_intersect beside the ad_parts_union that produced its input, and beside the host copy-back it replaces.

Input: the union of --replicas full-range replicas of synth.config3 (elision on / off alternating), rank-format ids.
Timed with the destinations' ranges a random split of the token space into --dest lists and one key route per
request (its keys):
  union       ad_parts_union of the replicas' parts (its own HIP events, ad_merged.ms_device, and the host clock)
  intersect   ad_deps_intersect of that ad_merged (HIP events around everything the call enqueues, its one host
              round trip included, ad_merged.ms_device; and the host clock around the call, which ends synchronised)
  copy_back   ad_copy_to_host of the merged arrays: what a host that slices on its store thread must do first

  python scripts/bench_intersect.py [--txns 200000 --keys 30000 --replicas 3 --dest 3 --warmup 3 --reps 20]

Prints one JSON line per measurement and a summary line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cassandra-accord_amd"))

from accord_deps import _abi as A  # noqa: E402
from accord_deps import exchange, native, synth  # noqa: E402


def med(xs):
    return round(float(np.median(xs)), 4)


def merged_bytes(mg):
    n, idb = mg.n_txns, 4 if mg.id_format == A.AD_IDS_RANK else 24
    b = 9 * 8 * (n + 1)
    for m in range(A.NMAPS):
        b += 8 * int(mg.n_keys[m]) * (2 if m == A.AD_MAP_RANGE else 1) + idb * int(mg.n_ids[m]) + 4 * int(mg.n_k2t[m])
    return b


def copy_back(st, mg):
    n = mg.n_txns
    for m in range(A.NMAPS):
        for p in (mg.keys_off[m], mg.txn_off[m], mg.k2t_off[m]):
            st._d2h(p, n + 1, np.uint64)
        st._d2h(mg.keys[m], int(mg.n_keys[m]) * (2 if m == A.AD_MAP_RANGE else 1), np.int64)
        if mg.id_format == A.AD_IDS_RANK:
            st._d2h(mg.txns[m], int(mg.n_ids[m]), np.uint32)
        else:
            st._d2h(mg.txns[m], 3 * int(mg.n_ids[m]), np.int64)
        st._d2h(mg.k2t[m], int(mg.n_k2t[m]), np.int32)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=200_000)
    ap.add_argument("--keys", type=int, default=30_000)
    ap.add_argument("--replicas", type=int, default=3)
    ap.add_argument("--dest", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_intersect.py needs a GPU"
    dev = torch.device("cuda", 0)
    t0 = time.time()
    w = synth.config3(n_txns=a.txns, n_keys=a.keys, seed=77)
    n = len(w.queries)
    reps = []
    for i in range(a.replicas):
        st = native.DeviceCommandStore(0, w.range_start_inclusive, i % 2, w.slices)
        st.load(w)
        qdev, keep = native.device_queries(w.queries, dev)
        reps.append((exchange.GpuEngine(st, qdev, np.arange(n), dev), keep))
    g = exchange.build_global_dict([r[0].dictionary() for r in reps])
    sends = []
    for eng, _ in reps:
        eng.set_global_dict(g)
    for eng, _ in reps:
        eng.resolve()
        sends.append(eng.export(np.array([0, n], np.uint64)))
    torch.cuda.synchronize()
    recv, totals = {}, np.zeros(4, np.int64)
    for k, (name, mult) in enumerate((("hdr", 4), ("keys", 1), ("ids", 1), ("k2t", 1))):
        recv[name] = torch.cat([s[0][name][:int(s[1][0, k]) * mult] for s in sends])
    for s in sends:
        totals += s[1][0]
    p = A.AdParts()
    p.hdr, p.keys, p.ids, p.k2t = (recv[k].data_ptr() for k in ("hdr", "keys", "ids", "k2t"))
    p.n_parts, p.n_key_words, p.n_ids, p.n_k2t = (int(x) for x in totals)
    p.id_format = A.AD_IDS_RANK
    src = [int(s[1][0, 0]) for s in sends]
    routes, dest = synth.deps_scopes(w, a.dest, 1, two_ranges=True, empty_dest=False, drop_frac=0.0)
    rt = [torch.from_numpy(np.append(routes.domain, np.uint8(0))).to(dev),
          torch.from_numpy(np.append(routes.off, np.uint64(0)).view(np.int64)).to(dev),
          torch.from_numpy(np.append(routes.words, np.int64(0))).to(dev)]
    torch.cuda.synchronize()
    rptr = tuple(t.data_ptr() for t in rt)
    print("# set-up %.1fs: %d requests, %d replicas, %d destinations" % (time.time() - t0, n, a.replicas, a.dest), flush=True)
    owner = reps[0][0].store

    def timed(f):
        dev_ms, host_ms, last = [], [], None
        for i in range(a.warmup + a.reps):
            t = time.perf_counter()
            last = f()
            h = (time.perf_counter() - t) * 1e3
            if i >= a.warmup:
                dev_ms.append(last.ms_device)
                host_ms.append(h)
        return dev_ms, host_ms, last

    ud, uh, mg = timed(lambda: owner.union_parts(p, src, 0, n))
    in_b = merged_bytes(mg)
    print(json.dumps(dict(what="ad_parts_union", ms_device=med(ud), ms_device_min=round(min(ud), 4),
                          ms_device_max=round(max(ud), 4), ms_host=med(uh), out_bytes=in_b,
                          ids=[int(x) for x in mg.n_ids], keys=[int(x) for x in mg.n_keys])), flush=True)
    xd, xh, out = timed(lambda: owner.intersect_merged(mg, dest, rptr))
    out_b = merged_bytes(out)
    print(json.dumps(dict(what="ad_deps_intersect", n_dest=a.dest, ms_device=med(xd), ms_device_min=round(min(xd), 4),
                          ms_device_max=round(max(xd), 4), ms_host=med(xh), in_bytes=in_b, out_bytes=out_b,
                          ids=[int(x) for x in out.n_ids], keys=[int(x) for x in out.n_keys])), flush=True)
    cb = []
    for i in range(a.warmup + a.reps):
        t = time.perf_counter()
        copy_back(owner, mg)
        if i >= a.warmup:
            cb.append((time.perf_counter() - t) * 1e3)
    print(json.dumps(dict(what="copy_back", ms_host=med(cb), bytes=in_b)), flush=True)
    print(json.dumps(dict(metric="deps_intersect", requests=n, n_dest=a.dest, union_ms_device=med(ud),
                          intersect_ms_device=med(xd), intersect_ms_host=med(xh), copy_back_ms_host=med(cb),
                          intersect_over_union=round(med(xd) / max(med(ud), 1e-9), 3), in_bytes=in_b, out_bytes=out_b,
                          gb_per_s=round((in_b * a.dest + out_b) / max(med(xd), 1e-9) / 1e6, 2))), flush=True)
    for eng, _ in reps:
        eng.store.close()


if __name__ == "__main__":
    main()
