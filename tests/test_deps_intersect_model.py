"""model.deps_intersecting (the CPU restatement ad_deps_intersect is tested against) checked on its own: against a
pair-set brute force in the style of KeyDepsTest.java:337-346 / RangeDepsTest.java:95-169 (flatten to (key or
range, txnId) pairs, filter by the scope predicate, rebuild the canonical form), by the lossless round trip of
the key maps over a partition of the token space, and on hand-made edge cases."""
import numpy as np
import pytest

import pyoracle
from accord_deps import _abi as A
from accord_deps import model, synth
from accord_deps.model import DepsMap, PartialDepsBatch, Routes, Tids

LO, HI = -(1 << 63), (1 << 63) - 1


def _map_equal(a, b):
    cols = [(a.keys_off, b.keys_off), (a.keys, b.keys), (a.txn_off, b.txn_off), (a.txn.msb, b.txn.msb),
            (a.txn.lsb, b.txn.lsb), (a.txn.node, b.txn.node), (a.k2t_off, b.k2t_off), (a.k2t, b.k2t)]
    if a.keys_end is not None or b.keys_end is not None:
        cols.append((a.keys_end, b.keys_end))
    return all(x is not None and y is not None and x.shape == y.shape and np.array_equal(x, y) for x, y in cols)


def _in(s, e, k, si):
    return (s <= k < e) if si else (s < k <= e)


def brute_force(batch, routes, dest_ranges, si):
    """Per (destination, request, map): the (key, id) pairs whose key the scope selects, rebuilt as
    keys ascending / ids ascending / keysToTxnIds = end offsets then lists. Rows as [(keys, ids, k2t)] * 3."""
    rows = []
    for rd in dest_ranges:
        rd = [(int(s), int(e)) for s, e in np.asarray(rd, np.int64).reshape(-1, 2)]
        for r in range(batch.n_txns):
            is_range, items = routes.of(r)
            row = []
            for m in range(A.NMAPS):
                ks, ke, t, k2t = batch.maps[m].request(r)
                nk = len(ks)
                pairs = set()
                for i in range(nk):
                    key = (int(ks[i]), int(ke[i])) if m == A.AD_MAP_RANGE else int(ks[i])
                    for v in k2t[(nk if i == 0 else k2t[i - 1]):k2t[i]]:
                        pairs.add((key, int(v)))

                def selected(key):
                    for ds, de in rd:
                        for it in items:
                            if m != A.AD_MAP_RANGE and not is_range:
                                if it == key and _in(ds, de, it, si):
                                    return True
                            elif m != A.AD_MAP_RANGE:
                                s, e = max(it[0], ds), min(it[1], de)
                                if s < e and _in(s, e, key, si):
                                    return True
                            elif not is_range:
                                if _in(ds, de, it, si) and _in(key[0], key[1], it, si):
                                    return True
                            else:
                                s, e = max(it[0], ds), min(it[1], de)
                                if s < e and s < key[1] and e > key[0]:
                                    return True
                    return False
                pairs = {p for p in pairs if selected(p[0])}
                keys = sorted({p[0] for p in pairs})
                ids = sorted({p[1] for p in pairs})
                pos = {v: j for j, v in enumerate(ids)}
                heads, lists = [], []
                for k in keys:
                    lists += sorted(pos[v] for kk, v in pairs if kk == k)
                    heads.append(len(keys) + len(lists))
                row.append((keys, t.take(np.asarray(ids, np.int64)).tuples(), heads + lists))
            rows.append(row)
    return rows


def rows_of(out):
    rows = []
    for i in range(out.n_txns):
        row = []
        for m in range(A.NMAPS):
            ks, ke, t, k2t = out.maps[m].request(i)
            keys = list(zip(ks.tolist(), ke.tolist())) if m == A.AD_MAP_RANGE else ks.tolist()
            row.append((keys, t.tuples(), k2t.tolist()))
        rows.append(row)
    return rows


def _check_brute(w, n_dest, seed, **kw):
    batch = pyoracle.resolve(w)
    routes, dest = synth.deps_scopes(w, n_dest, seed, **kw)
    got = model.deps_intersecting(batch, routes, dest, w.range_start_inclusive)
    assert got.n_txns == n_dest * batch.n_txns
    exp = brute_force(batch, routes, dest, w.range_start_inclusive)
    have = rows_of(got)
    for i, (a, b) in enumerate(zip(have, exp)):
        assert a == b, "row %d (destination %d, request %d)" % (i, i // batch.n_txns, i % batch.n_txns)
    return batch, got


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("n_dest", [1, 3])
def test_random_small_equals_brute_force(oracle, seed, n_dest):
    w = synth.random_small(700 + seed, range_frac=0.25 if seed % 2 else 0.0, start_inclusive=bool(seed & 2))
    batch, got = _check_brute(w, n_dest, seed, range_route_frac=0.3)
    assert sum(len(m.keys) for m in got.maps) > 0


def test_config4_small_equals_brute_force(oracle):
    w = synth.config4(n_txns=150, n_keys=200, n_ranges=60, n_hist_txns=300)
    w = synth.with_range_requests(w, 0.2)
    batch, got = _check_brute(w, 3, 9, drop_frac=0.1)
    assert len(got.maps[A.AD_MAP_RANGE].keys) > 0 and len(got.maps[A.AD_MAP_KEY].keys) > 0


@pytest.mark.parametrize("seed", range(4))
def test_key_maps_round_trip_over_a_partition(oracle, seed):
    """The destinations partition the token space and every route holds its request's keys: the rows of a request
    over all destinations merge (PartialDeps.with) back into the input's keyDeps and directKeyDeps."""
    w = synth.random_small(740 + seed, range_frac=0.3, start_inclusive=bool(seed & 1))
    batch = pyoracle.resolve(w)
    n = batch.n_txns
    routes, dest = synth.deps_scopes(w, 4, seed, empty_dest=False, drop_frac=0.0)
    got = model.deps_intersecting(batch, routes, dest, w.range_start_inclusive)
    back = pyoracle.merge_batches([got.window(d * n, n) for d in range(4)])
    for m in (A.AD_MAP_KEY, A.AD_MAP_DIRECT_KEY):
        assert _map_equal(back.maps[m], batch.maps[m]), A.MAP_NAMES[m]
    assert len(batch.maps[A.AD_MAP_KEY].keys) > 0


# ---- hand-made edge cases -------------------------------------------------------------------------------------

def _one(keymap, rangemap, n_ids):
    """A one-request batch: keymap {key: [id index]}, rangemap {(s, e): [id index]}, directKeyDeps empty."""
    ids = model.make_txn_ids(1, np.arange(100, 100 + n_ids), A.KIND_WRITE, 1)

    def cols(mp, used):
        keys = sorted(mp)
        idx = sorted(used)
        pos = {v: j for j, v in enumerate(idx)}
        heads, lists = [], []
        for k in keys:
            lists += [pos[v] for v in sorted(mp[k])]
            heads.append(len(keys) + len(lists))
        return keys, ids.take(np.asarray(idx, np.int64)), heads + lists
    maps = []
    for m, mp in ((0, keymap), (1, rangemap), (2, {})):
        keys, t, k2t = cols(mp, {v for vs in mp.values() for v in vs})
        ks = np.array([k[0] for k in keys] if m == 1 else keys, np.int64)
        ke = np.array([k[1] for k in keys], np.int64) if m == 1 else None
        maps.append(DepsMap(np.array([0, len(keys)], np.uint64), ks, ke, np.array([0, len(t)], np.uint64), t,
                            np.array([0, len(k2t)], np.uint64), np.array(k2t, np.int32)))
    return PartialDepsBatch(maps)


KEYMAP = {10: [0, 1], 20: [1], 30: [2, 3]}
RANGEMAP = {(0, 15): [0], (12, 40): [1, 2], (50, 60): [3]}


def _row(out, i, m):
    ks, ke, t, k2t = out.maps[m].request(i)
    keys = list(zip(ks.tolist(), ke.tolist())) if m == 1 else ks.tolist()
    return keys, [x[1] >> 16 for x in t.tuples()], k2t.tolist()


def test_empty_destination_and_nothing_selected():
    b = _one(KEYMAP, RANGEMAP, 4)
    routes = Routes.from_lists([(False, [10, 20, 30, 55])])
    out = model.deps_intersecting(b, routes, [np.zeros((0, 2), np.int64), np.array([[100, 200]])], 0)
    for i in (0, 1):
        for m in range(3):
            assert _row(out, i, m) == ([], [], [])


def test_everything_selected_is_identity():
    b = _one(KEYMAP, RANGEMAP, 4)
    routes = Routes.from_lists([(True, [(LO, HI)])])
    out = model.deps_intersecting(b, routes, [np.array([[LO, HI]])], 0)
    ok, why = out.equals(b, detail=True)
    assert ok, why


def test_trim_and_remap():
    b = _one(KEYMAP, RANGEMAP, 4)
    routes = Routes.from_lists([(False, [20, 30])])
    out = model.deps_intersecting(b, routes, [np.array([[LO, HI]])], 0)
    # keys 20 -> {id 1}, 30 -> {ids 2, 3}: ids 101, 102, 103 kept, indices shifted down by one
    assert _row(out, 0, 0) == ([20, 30], [101, 102, 103], [3, 5, 0, 1, 2])


def test_range_without_route_key_dropped_under_key_route_kept_under_range_route():
    b = _one({}, RANGEMAP, 4)
    dest = [np.array([[45, 70]])]
    # (50, 60) lies in R_d; the key route has no key in it
    out = model.deps_intersecting(b, Routes.from_lists([(False, [13, 48])]), dest, 0)
    assert _row(out, 0, 1) == ([], [], [])
    out = model.deps_intersecting(b, Routes.from_lists([(True, [(0, 100)])]), dest, 0)
    assert _row(out, 0, 1) == ([(50, 60)], [103], [2, 0])
    # with a route key inside it, it is kept, whole
    out = model.deps_intersecting(b, Routes.from_lists([(False, [13, 55])]), dest, 0)
    assert _row(out, 0, 1) == ([(50, 60)], [103], [2, 0])


def test_range_spanning_two_destinations_is_in_both():
    b = _one({}, RANGEMAP, 4)
    dest = [np.array([[0, 20]]), np.array([[20, 45]])]
    out = model.deps_intersecting(b, Routes.from_lists([(True, [(0, 100)])]), dest, 0)
    assert _row(out, 0, 1) == ([(0, 15), (12, 40)], [100, 101, 102], [3, 5, 0, 1, 2])
    assert _row(out, 1, 1) == ([(12, 40)], [101, 102], [3, 0, 1])
    out = model.deps_intersecting(b, Routes.from_lists([(False, [14, 30])]), dest, 0)
    assert _row(out, 0, 1)[0] == [(0, 15), (12, 40)] and _row(out, 1, 1)[0] == [(12, 40)]


@pytest.mark.parametrize("si", [0, 1])
def test_key_exactly_on_a_boundary(si):
    b = _one(KEYMAP, RANGEMAP, 4)
    dest = [np.array([[0, 20]]), np.array([[20, 40]])]
    out = model.deps_intersecting(b, Routes.from_lists([(False, [10, 20, 30])]), dest, si)
    # key 20: in (0, 20] when ends are inclusive, in [20, 40) when starts are
    assert _row(out, 0, 0)[0] == ([10] if si else [10, 20])
    assert _row(out, 1, 0)[0] == ([20, 30] if si else [30])
    # route key 12 against the range (12, 40): its start holds 12 only when starts are inclusive
    out = model.deps_intersecting(b, Routes.from_lists([(False, [12])]), [np.array([[0, 100]])], si)
    assert _row(out, 0, 1)[0] == ([(0, 15), (12, 40)] if si else [(0, 15)])
    # a range route (0, 10) against key 10 and against the range (12, 40): bounds that only touch never intersect
    out = model.deps_intersecting(b, Routes.from_lists([(True, [(0, 10), (40, 50)])]), [np.array([[0, 100]])], si)
    assert _row(out, 0, 0)[0] == ([] if si else [10])
    assert _row(out, 0, 1)[0] == [(0, 15)]
