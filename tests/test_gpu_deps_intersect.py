"""GPU parity of ad_deps_intersect (Deps.intersecting of the coordinator's merged deps, per replica): the merged
input is built on the GPU -- rank format as test_gpu_union.py does (small replicas, then union_parts), triplet
format by merge_parts of hand-exported parts on a store with no dictionary -- and
merged_to_host(intersect_merged(..)) is compared bit-exactly with model.deps_intersecting applied to
merged_to_host(mg). ad_check_result_device validates the ad_deps_result layout (snapshot ranks, range-table
ids), not ad_merged, so the result's structure is checked on the host here (_check_structure)."""
import numpy as np
import pytest
import torch

import pyoracle
from accord_deps import _abi as A
from accord_deps import exchange, model, native, synth
from accord_deps.model import Routes

pytestmark = pytest.mark.gpu

FULL = (-(1 << 63), (1 << 63) - 1)
_open = []


@pytest.fixture(scope="module", autouse=True)
def _close_stores():
    yield
    while _open:
        _open.pop().close()
    _union_cached.cache.clear()


def _union(w, bounds, elides):
    """The union of the replicas' answers on the first replica's store (rank format): (store, AdMerged)."""
    dev = torch.device("cuda", 0)
    n = len(w.queries)
    reps = []
    for (lo, hi), e in zip(bounds, elides):
        ws = synth.slice_workload(w, lo, hi)
        st = native.DeviceCommandStore(0, w.range_start_inclusive, e, ws.slices)
        _open.append(st)
        st.load(ws)
        qdev, keep = native.device_queries(ws.queries, dev)
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
    for a, (name, mult) in enumerate((("hdr", 4), ("keys", 1), ("ids", 1), ("k2t", 1))):
        recv[name] = torch.cat([s[0][name][:int(s[1][0, a]) * mult] for s in sends])
    for s in sends:
        totals += s[1][0]
    p = A.AdParts()
    p.hdr, p.keys, p.ids, p.k2t = (recv[k].data_ptr() for k in ("hdr", "keys", "ids", "k2t"))
    p.n_parts, p.n_key_words, p.n_ids, p.n_k2t = (int(x) for x in totals)
    p.id_format = A.AD_IDS_RANK
    owner = reps[0][0].store
    mg = owner.union_parts(p, [int(s[1][0, 0]) for s in sends], 0, n)
    for eng, _ in reps[1:]:
        eng.store.close()
    return owner, mg


def _union_cached(key, make):
    if key not in _union_cached.cache:
        w = make()
        _union_cached.cache[key] = (w,) + _union(w, *_REPLICAS[key[0]])
    return _union_cached.cache[key]


_union_cached.cache = {}
_REPLICAS = {
    "small": ([(-(1 << 63), 150), (-200, (1 << 63) - 1), FULL], [1, 0, 1]),
    "config4": ([FULL, FULL], [1, 0]),
    "big": ([FULL, FULL, (-(1 << 62), 1 << 62)], [1, 0, 1]),
}


def _merge_triplets(batch, start_inclusive=0):
    """`batch` (a host PartialDepsBatch) exported by hand as triplet-format parts and merged by a store with
    nothing loaded and no global dictionary: (store, AdMerged with id_format TRIPLET)."""
    dev = torch.device("cuda", 0)
    hdr, keys, ids, k2t = [], [], [], []
    for r in range(batch.n_txns):
        for m in range(A.NMAPS):
            ks, ke, t, o = batch.maps[m].request(r)
            if not len(ks):
                continue
            hdr += [(r << 2) | m, len(ks), len(t), len(o)]
            keys += np.stack([ks, ke], 1).reshape(-1).tolist() if m == A.AD_MAP_RANGE else ks.tolist()
            ids += np.stack([t.msb.view(np.int64), t.lsb.view(np.int64), t.node.astype(np.int64)], 1).reshape(-1).tolist()
            k2t += o.tolist()
    ten = [torch.tensor(x + [0], dtype=dt).to(dev) for x, dt in ((hdr, torch.int64), (keys, torch.int64),
                                                                (ids, torch.int64), (k2t, torch.int32))]
    torch.cuda.synchronize()
    p = A.AdParts()
    p.hdr, p.keys, p.ids, p.k2t = (x.data_ptr() for x in ten)
    p.n_parts, p.n_key_words, p.n_ids, p.n_k2t = len(hdr) // 4, len(keys), len(ids) // 3, len(k2t)
    p.id_format = A.AD_IDS_TRIPLET
    st = native.DeviceCommandStore(0, start_inclusive)
    _open.append(st)
    return st, st.merge_parts(p, [p.n_parts], 0, batch.n_txns)


def _check_structure(out):
    """RelationMultiMap's invariants on every row (checkValid, RelationMultiMap.java): keys and ids strictly
    ascending, end offsets ascending from the key count to the length, lists strictly ascending id indices."""
    for i in range(out.n_txns):
        for m in range(A.NMAPS):
            ks, ke, t, o = out.maps[m].request(i)
            nk, o = len(ks), o.tolist()
            keys = list(zip(ks.tolist(), ke.tolist())) if ke is not None else ks.tolist()
            assert all(a < b for a, b in zip(keys, keys[1:])), (i, m)
            order = [model.tid_order(x) for x in t.tuples()]
            assert all(a < b for a, b in zip(order, order[1:])), (i, m)
            if nk == 0:
                assert len(t) == 0 and o == [], (i, m)
                continue
            assert o[nk - 1] == len(o), (i, m)
            seen = set()
            for k in range(nk):
                lst = o[(nk if k == 0 else o[k - 1]):o[k]]
                assert lst and all(a < b for a, b in zip(lst, lst[1:])) and 0 <= lst[0] and lst[-1] < len(t), (i, m)
                seen.update(lst)
            assert len(seen) == len(t), (i, m)


def _compare(st, mg, routes, dest, start_inclusive, structure=True):
    before = st.merged_to_host(mg)
    out = st.intersect_merged(mg, dest, routes)
    got = st.merged_to_host(out)
    assert out.n_txns == len(dest) * mg.n_txns and out.id_format == mg.id_format
    exp = model.deps_intersecting(before, routes, dest, start_inclusive)
    ok, why = got.equals(exp, detail=True)
    assert ok, "%s; first mismatch %s" % (why, got.first_mismatch(exp))
    after = st.merged_to_host(mg)
    ok, why = after.equals(before, detail=True)
    assert ok, "the input ad_merged changed: %s" % why
    if structure:
        _check_structure(got)
    return before, got


@pytest.mark.parametrize("n_dest", [1, 3, 8])
@pytest.mark.parametrize("seed", range(3))
def test_random_small_key_routes(seed, n_dest):
    def make():
        w = synth.random_small(400 + seed)
        w.slices = None
        return w
    w, st, mg = _union_cached(("small", seed), make)
    # one destination owns two disjoint ranges; with more than one destination, one owns none
    routes, dest = synth.deps_scopes(w, n_dest, 50 + seed)
    assert max(len(d) for d in dest) == 2 and (n_dest == 1 or min(len(d) for d in dest) == 0)
    before, got = _compare(st, mg, routes, dest, w.range_start_inclusive)
    assert sum(len(m.keys) for m in got.maps) > 0


@pytest.mark.parametrize("seed", range(2))
def test_random_small_range_routes_start_inclusive(seed):
    def make():
        w = synth.random_small(430 + seed, range_frac=0.3, start_inclusive=True)
        w.slices = None
        return w
    w, st, mg = _union_cached(("small", 100 + seed), make)
    routes, dest = synth.deps_scopes(w, 3, 60 + seed, range_route_frac=0.4)
    assert routes.domain.any() and not routes.domain.all()
    _compare(st, mg, routes, dest, w.range_start_inclusive)


def test_config4_key_and_range_routes():
    def make():
        return synth.with_range_requests(synth.config4(n_txns=2000, n_keys=3000, n_ranges=600, n_hist_txns=2000), 0.1)
    w, st, mg = _union_cached(("config4", 0), make)
    routes, dest = synth.deps_scopes(w, 3, 7, drop_frac=0.1)
    assert routes.domain.any() and not routes.domain.all()
    before, got = _compare(st, mg, routes, dest, w.range_start_inclusive, structure=False)
    assert len(got.maps[A.AD_MAP_RANGE].keys) > 0 and len(got.maps[A.AD_MAP_KEY].keys) > 0


def test_big_groups():
    """Hot keys: every keyDeps of this shape holds hundreds to thousands of ids (none of 64 or fewer -- those are
    test_id_count_boundaries' and the other tests'), so every group takes the block kernel."""
    def make():
        return synth.config2(n_txns=200, n_keys=40, n_hist_entries=40000, keys_per_txn=8, tail_unapplied=300)
    w, st, mg = _union_cached(("big", 0), make)
    routes, dest = synth.deps_scopes(w, 3, 11, drop_frac=0.3)
    before, got = _compare(st, mg, routes, dest, w.range_start_inclusive, structure=False)
    to = before.maps[A.AD_MAP_KEY].txn_off.astype(np.int64)
    n_ids = to[1:] - to[:-1]
    oo = before.maps[A.AD_MAP_KEY].k2t_off.astype(np.int64)
    n_k2t = oo[1:] - oo[:-1]
    # the model's input really holds maps of several hundred ids and more, beyond what the one-wave kernel takes
    # (2048 ids, 4096 keysToTxnIds ints)
    assert (n_ids >= 300).all() and ((n_k2t > 4096) | (n_ids > 2048)).any(), (int(n_ids.min()), int(n_k2t.max()))


def _boundary_batch(counts, n_keys=5, seed=3):
    """One request per entry of counts: a keyDeps of n_keys keys over exactly that many ids, every id named."""
    rng = np.random.default_rng(seed)
    ids = model.make_txn_ids(1, np.arange(1000, 1000 + max(counts)), A.KIND_WRITE, 1)
    ko, keys, to, tix, oo, k2t = [0], [], [0], [], [0], []
    for c in counts:
        nk = min(n_keys, c)
        owner = rng.integers(0, nk, c)
        owner[:nk] = np.arange(nk)                    # every key names an id
        extra = rng.random((nk, c)) < 0.3
        heads, lists = [], []
        for k in range(nk):
            lst = np.flatnonzero((owner == k) | extra[k]).tolist()
            lists += lst
            heads.append(nk + len(lists))
        keys += (10 * np.arange(nk)).tolist()
        tix += list(range(c))
        k2t += heads + lists
        ko.append(len(keys)); to.append(len(tix)); oo.append(len(k2t))
    z = np.zeros(len(counts) + 1, np.uint64)
    e64, e32 = np.zeros(0, np.int64), np.zeros(0, np.int32)
    none = model.Tids(np.zeros(0, np.uint64), np.zeros(0, np.uint64), e32)
    km = model.DepsMap(np.array(ko, np.uint64), np.array(keys, np.int64), None, np.array(to, np.uint64),
                       ids.take(np.asarray(tix, np.int64)), np.array(oo, np.uint64), np.array(k2t, np.int32))
    return model.PartialDepsBatch([km, model.DepsMap(z, e64, e64, z, none, z, e32), model.DepsMap(z, e64, None, z, none, z, e32)])


def test_id_count_boundaries():
    counts = [1, 31, 32, 33, 63, 64, 65, 300, 2047, 2048, 2049, 2500]
    batch = _boundary_batch(counts)
    to = batch.maps[0].txn_off.astype(np.int64)
    assert (to[1:] - to[:-1]).tolist() == counts
    st, mg = _merge_triplets(batch)
    assert mg.id_format == A.AD_IDS_TRIPLET
    # keys 0, 10, 20, 30, 40: the route drops 20, the destinations cut between 10 and 30
    routes = Routes.from_lists([(False, [0, 10, 30, 40])] * len(counts))
    dest = [np.array([[-5, 15]]), np.array([[15, 100]])]
    before, got = _compare(st, mg, routes, dest, 0)
    kept = got.maps[0].txn_off.astype(np.int64)
    assert ((kept[1:] - kept[:-1])[:len(counts)] < np.array(counts))[2:].all()      # ids were trimmed


@pytest.mark.parametrize("seed", range(2))
def test_triplet_input(oracle, seed):
    w = synth.random_small(460 + seed, range_frac=0.3)
    st, mg = _merge_triplets(pyoracle.resolve(w), w.range_start_inclusive)
    assert mg.id_format == A.AD_IDS_TRIPLET
    routes, dest = synth.deps_scopes(w, 3, 80 + seed, range_route_frac=0.3)
    _compare(st, mg, routes, dest, w.range_start_inclusive)


def test_identity_and_empty_rows(oracle):
    w = synth.random_small(470, range_frac=0.3)
    batch = pyoracle.resolve(w)
    st, mg = _merge_triplets(batch, w.range_start_inclusive)
    n = batch.n_txns
    # every route is the whole token space; destination 0 owns it all, destination 1 nothing, destination 2 a
    # range beyond every key
    routes = Routes.from_lists([(True, [FULL])] * n)
    dest = [np.array([FULL]), np.zeros((0, 2), np.int64), np.array([[1 << 40, 1 << 41]])]
    before, got = _compare(st, mg, routes, dest, w.range_start_inclusive)
    ok, why = got.window(0, n).equals(before, detail=True)
    assert ok, "selecting everything must reproduce the input: %s" % why
    for m in got.maps:
        assert int(m.keys_off[-1]) == int(m.keys_off[n]) and int(m.txn_off[-1]) == int(m.txn_off[n])
        assert int(m.k2t_off[-1]) == int(m.k2t_off[n])
    assert sum(len(m.keys) for m in before.maps) > 0


def test_errors_leave_the_store_usable(oracle):
    w = synth.random_small(480)
    batch = pyoracle.resolve(w)
    st, mg = _merge_triplets(batch, w.range_start_inclusive)
    routes, dest = synth.deps_scopes(w, 2, 5, empty_dest=False, two_ranges=False)
    for bad in ([np.array([[0, 100], [50, 200]])] + dest[1:],          # overlapping
                [np.array([[100, 200], [0, 50]])] + dest[1:],          # unsorted
                [np.array([[7, 7]])] + dest[1:]):                      # empty range
        with pytest.raises(native.AccordDepsError) as ei:
            st.intersect_merged(mg, bad, routes)
        assert ei.value.code == A.AD_E_INVAL
    shifted = Routes(routes.domain, routes.off + np.uint64(1), np.concatenate([[0], routes.words]))
    with pytest.raises(native.AccordDepsError) as ei:
        st.intersect_merged(mg, dest, shifted)
    assert ei.value.code == A.AD_E_INVAL
    with pytest.raises(native.AccordDepsError) as ei:
        st.intersect_merged(mg, dest, (None, None, None))
    assert ei.value.code == A.AD_E_INVAL
    _compare(st, mg, routes, dest, w.range_start_inclusive)
