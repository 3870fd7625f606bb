"""GPU parity of ad_redundant_merge: the store's RedundantBefore replaced in place by the host's
RedundantBefore.merge result (RedundantBefore.java:375-377) -- entries split, joined, added over gaps -- without a
snapshot rebuild. A stateful oracle store runs alongside the device store: rc_redundant_load on a live store
replaces its entries and its next read truncates to them (refcpu.c store_truncate). Truncation steps do not
commute where missing() lists are held (the trim happens only where entries left), so both sides read after
every merge."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from accord_deps import _abi as A
from accord_deps import native, synth
from accord_deps.model import CfkUpdates, Queries, Redundant, Tids, make_txn_ids

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

pytestmark = pytest.mark.gpu


def _small(seed, **kw):
    kw.setdefault("n_redundant", 3 + seed % 5)
    return synth.random_small(seed, n_keys=50, n_hist_txns=400, n_txns=150, **kw)


def _with(w, red=None, cfk=None, cmds=None):
    return type(w)(w.name, cfk or w.cfk, cmds or w.cmds, red or w.redundant, w.queries, w.flags, w.params,
                   w.range_start_inclusive, w.slices)


class Pair:
    """A device store and an oracle store loaded alike, driven in lockstep."""

    def __init__(self, w, path=0, prepare=True):
        import pyoracle
        self.py, self.w = pyoracle, w
        self.st = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices, path=path)
        self.orc = pyoracle.OracleStore(w.range_start_inclusive, 1, w.slices)
        self.st.load(w, prepare=prepare)
        self.orc.load(w)

    def close(self):
        self.st.close()
        self.orc.close()

    def merge(self, red):
        stats = self.st.redundant_merge(red)
        rc = self.py.lib().rc_redundant_load(self.orc.h, C.byref(red.soa()))
        assert rc == 0
        return stats

    def read(self, tag=None):
        got = self.st.calculate_partial_deps(self.w.queries, self.w.flags)
        exp = self.orc.deps_batch(self.w.queries, self.w.flags)
        ok, why = got.equals(exp, detail=True)
        assert ok, (tag, why, got.first_mismatch(exp))
        return got

    def views(self, cfk):
        """cfk_byid / cfk_entries / cfk_missing against the generator's truncated store `cfk`"""
        keys, seg, txn, pruned = self.st.cfk_byid()
        assert keys.tolist() == cfk.keys.tolist() and seg.tolist() == cfk.seg.tolist()
        assert txn.tuples() == cfk.txn.tuples()
        if cfk.pruned_before is not None:
            assert pruned.tolist() == cfk.pruned_before.tolist()
        s, x = self.st.cfk_entries()
        assert s.tolist() == cfk.status.tolist() and x.tuples() == cfk.exec.tuples()
        if cfk.miss_off is not None:
            off, m = self.st.cfk_missing()
            assert off.tolist() == cfk.miss_off.tolist() and m.tuples() == cfk.miss.tuples()
        assert self.st.check_snapshot()[0] == 0


def _keys_in(w, i):
    """the store's keys inside RedundantBefore entry i"""
    s, e = int(w.redundant.range_start[i]), int(w.redundant.range_end[i])
    k = w.cfk.keys
    return k[(k >= s) & (k < e)] if w.range_start_inclusive else k[(k > s) & (k <= e)]


def _split_on_keys(w, seed, hist):
    """a split of the entry holding the most keys, its new boundaries exactly on two of them"""
    n = len(w.redundant.range_start)
    i = max(range(n), key=lambda j: len(_keys_in(w, j)))
    ks = _keys_in(w, i)
    s, e = int(w.redundant.range_start[i]), int(w.redundant.range_end[i])
    inner = [int(k) for k in ks if s < k < e]
    assert len(inner) >= 2, "the widest entry holds too few keys for this case"
    a, b = inner[len(inner) // 4], inner[(3 * len(inner)) // 4]
    assert a < b
    return synth.merge_redundant(w.redundant, seed, ranges=[(a, b)], hist_hlc=hist, step_frac=0.5)


@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("incl", [False, True])
@pytest.mark.parametrize("seed", range(3))
def test_split_then_join(oracle, seed, incl, path):
    w = _small(6000 + seed, start_inclusive=incl, n_redundant=4 + seed)
    hist = int(synth._hlc(w.cfk.txn).max())
    p = Pair(w, path)
    try:
        p.read("loaded")
        n0 = len(w.redundant.range_start)
        red1 = _split_on_keys(w, seed, hist)
        assert len(red1.range_start) == n0 + 2
        stats = p.merge(red1)
        assert stats["ms_stage"][1] > 0 and 0 < stats["n_probes"] < len(w.cfk.keys)
        p.read("split")
        cfk1 = synth.truncate_to_redundant(w.cfk, red1, incl)
        p.views(cfk1)
        # the neighbour advances to the same watermark and epochs: the entries join
        red2 = synth.merge_redundant(red1, seed, "join")
        assert len(red2.range_start) == n0 + 1
        p.merge(red2)
        p.read("join")
        p.views(synth.truncate_to_redundant(cfk1, red2, incl))
    finally:
        p.close()


def test_gap_fill_and_span(oracle):
    w = _small(6100, n_redundant=5)
    hist = int(synth._hlc(w.cfk.txn).max())
    p = Pair(w)
    try:
        p.read()
        red, cfk = w.redundant, w.cfk
        for step, mode in enumerate(("gap", "gap", "span")):
            red = synth.merge_redundant(red, 20 + step, mode, hist_hlc=hist, step_frac=0.3)
            stats = p.merge(red)
            assert stats["ms_stage"][1] > 0
            p.read(mode)
            cfk = synth.truncate_to_redundant(cfk, red, bool(w.range_start_inclusive))
            p.views(cfk)
        # the span left no gap between the first start and the last end
        assert red.range_end[:-1].tolist() == red.range_start[1:].tolist()
        assert cfk.n_entries < w.cfk.n_entries
    finally:
        p.close()


def test_from_empty_and_to_one(oracle):
    # a store loaded with an empty RedundantBefore receives its first entries, then one spanning entry
    full = _small(6200, n_redundant=4, truncated=False)
    w = _with(full, red=Redundant.empty())
    p = Pair(w)
    try:
        p.read()
        stats = p.merge(full.redundant)
        assert stats["ms_stage"][1] > 0 and stats["n_keys"][0] > 0
        p.read("first entries")
        cfk = synth.truncate_to_redundant(w.cfk, full.redundant, bool(w.range_start_inclusive))
        p.views(cfk)
        e = [(int(full.redundant.range_start[0]), int(full.redundant.range_end[-1]), 0, 1 << 40,
              make_txn_ids(9, np.array([5], np.uint64), A.KIND_EXCLUSIVE_SYNC_POINT, 3, domain=1).tuples()[0])]
        one = Redundant.from_entries(e)
        p.merge(one)
        p.read("one entry")
        p.views(synth.truncate_to_redundant(cfk, one, bool(w.range_start_inclusive)))
    finally:
        p.close()


@pytest.mark.parametrize("n_keys", [3, 6])
def test_long_segments(oracle, n_keys):
    # byId segments of hundreds of entries: 3 long keys in a wave are searched by the wave, one after the other;
    # 6 are more than it takes on, so every lane searches its own
    full = synth.random_small(6900 + n_keys, n_keys=n_keys, n_hist_txns=1200, n_txns=100, max_keys=3, n_redundant=2,
                              truncated=False)
    assert int(np.diff(full.cfk.seg.astype(np.int64)).min()) >= 128
    w = _with(full, red=Redundant.empty())
    by_id = np.lexsort(w.cfk.txn.order_key())
    p = Pair(w)
    try:
        p.read()
        cfk = w.cfk
        for step, frac in enumerate((0.3, 0.7)):
            at = w.cfk.txn.take(by_id[int(len(by_id) * frac):][:1])          # a watermark inside the history
            wm = make_txn_ids(at.epoch(), synth._hlc(at), A.KIND_EXCLUSIVE_SYNC_POINT, 3, domain=1).tuples()[0]
            lo = -520 if step == 0 else -600                   # the second step moves a boundary too
            red = Redundant.from_entries([(lo, 520, 0, 1 << 40, wm)])
            stats = p.merge(red)
            assert stats["n_probes"] == n_keys and stats["n_keys"][0] > 0
            p.read(step)
            cfk = synth.truncate_to_redundant(cfk, red, bool(w.range_start_inclusive))
            p.views(cfk)
    finally:
        p.close()


def test_to_empty(oracle):
    # the other direction: entries that hold nothing above NONE give way to an empty map (n_rb > 0 to 0); the
    # range table shrinks to the range commands' ranges
    w = _small(6250, n_redundant=4, n_range_cmds=10, range_frac=0.3)
    n = len(w.redundant.range_start)
    z = Tids(np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.int32))
    w = _with(w, red=Redundant(w.redundant.range_start, w.redundant.range_end, w.redundant.start_epoch,
                               w.redundant.end_epoch, z))
    p = Pair(w)
    try:
        p.read()
        stats = p.merge(Redundant.empty())
        assert stats["ms_stage"][1] > 0 and stats["n_keys"][0] == 0 and stats["n_probes"] == 0
        p.read("emptied")
        assert _table(p.st) == _expected_table(w.cmds, Redundant.empty())
        assert p.st.check_snapshot()[0] == 0
        # and entries again on top of the empty map
        full = _small(6250, n_redundant=4, n_range_cmds=10, range_frac=0.3).redundant
        p.merge(full)
        p.read("entries again")
        assert _table(p.st) == _expected_table(w.cmds, full)
    finally:
        p.close()


def _table(st):
    s, e = st.range_table()
    return list(zip(s.tolist(), e.tolist()))


def _expected_table(cmds, red):
    """ad_range_table: the sorted union of the scanned range commands' ranges (erased live ones are skipped) and
    the RedundantBefore ranges"""
    rs = set(zip(red.range_start.tolist(), red.range_end.tolist()))
    for i in range(len(cmds.txn)):
        hist = cmds.historical is not None and cmds.historical[i]
        if not hist and cmds.erased is not None and cmds.erased[i]:
            continue
        for r in range(int(cmds.range_off[i]), int(cmds.range_off[i + 1])):
            rs.add((int(cmds.range_start[r]), int(cmds.range_end[r])))
    return sorted(rs)


def _straddling(bounds, hlc):
    """Range-domain requests (a Write, a SyncPoint, an ExclusiveSyncPoint) whose ranges straddle, touch from either
    side and span the given boundaries"""
    b = sorted(bounds)
    ranges = [[(x - 3, x + 2) for x in b], [(b[0] - 4, b[0]), (b[0], b[0] + 4)], [(b[0] - 1, b[-1] + 1)]]
    kinds = np.array([A.KIND_WRITE, A.KIND_SYNC_POINT, A.KIND_EXCLUSIVE_SYNC_POINT], np.uint8)
    t = make_txn_ids(2, np.array([hlc + 11, hlc + 12, hlc + 13], np.uint64), kinds, 5, domain=1)
    off = np.cumsum([0] + [len(r) for r in ranges]).astype(np.uint64)
    flat = [x for r in ranges for x in r]
    return Queries(t, t, np.zeros(4, np.uint64), np.zeros(0, np.int64), np.zeros(3, np.int64), off,
                   np.array([x[0] for x in flat], np.int64), np.array([x[1] for x in flat], np.int64))


@pytest.mark.parametrize("path", [0, 1])
def test_range_table_follows(oracle, path):
    # range commands and Range-domain requests straddling the new boundaries: the RANGE map's range ids resolve
    # through ad_range_table (calculate_partial_deps materialises them) to the oracle's ranges
    w = _small(6300 + path, n_redundant=5, n_range_cmds=20, range_frac=0.3)
    hist = int(synth._hlc(w.cfk.txn).max())
    p = Pair(w, path)
    try:
        p.read()
        red = synth.merge_redundant(w.redundant, 1, "wm", hist_hlc=hist)
        stats = p.merge(red)
        assert stats["ms_stage"][1] == 0                 # watermarks only: the range part stands
        p.read("wm only")
        red = _split_on_keys(_with(w, red=red), 2, hist)
        stats = p.merge(red)
        assert stats["ms_stage"][1] > 0                  # boundaries changed: refreshed
        p.read("split")
        assert _table(p.st) == _expected_table(w.cmds, red)
        # requests built to straddle the two new boundaries
        new_bounds = sorted(set(red.range_start.tolist() + red.range_end.tolist()) -
                            set(w.redundant.range_start.tolist() + w.redundant.range_end.tolist()))
        assert len(new_bounds) == 2
        q = _straddling(new_bounds, int(synth._hlc(w.queries.txn).max()))
        got = p.st.calculate_partial_deps(q, w.flags)
        ok, why = got.equals(p.orc.deps_batch(q, w.flags), detail=True)
        assert ok, why
        assert int(got.maps[A.AD_MAP_RANGE].keys_off[-1]) > 0, "the straddling requests found range dependencies"
        red = synth.merge_redundant(red, 3, "gap", hist_hlc=hist)
        p.merge(red)
        p.read("gap")
        assert _table(p.st) == _expected_table(w.cmds, red)
        assert p.st.check_snapshot()[0] == 0
    finally:
        p.close()


@pytest.mark.parametrize("seed", range(3))
def test_sequential_after_merge(oracle, seed):
    # range transactions the new entries make shard-redundant register nothing (RedundantBefore.java:216-225)
    w = synth.sequential_ranges(6400 + seed, n_keys=40, n_txns=100, n_redundant=5, range_frac=0.3)
    hist = int(synth._hlc(w.queries.txn).max())
    p = Pair(w)
    try:
        red = synth.merge_redundant(w.redundant, seed, "split", hist_hlc=hist, step_frac=0.6)
        red = synth.merge_redundant(red, seed + 10, "gap", hist_hlc=hist, step_frac=0.6)
        p.merge(red)
        p.read("sequential")
    finally:
        p.close()


@pytest.mark.parametrize("device_lists", [False, True])
def test_recovery_two_merges(oracle, device_lists):
    w = synth.recovery_workload(6500, n_redundant=6)
    if device_lists:
        w.cfk = synth.with_missing(w.cfk, 6500)          # ids of byId only: the lists can move to the device
    hist = int(synth._hlc(w.cfk.txn).max())
    p = Pair(w)
    try:
        if device_lists:
            z = Tids(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.int32))
            p.st.cfk_update(CfkUpdates(np.zeros(0, np.int64), z, z, np.zeros(0, np.uint8), dep_off=np.zeros(1, np.uint64),
                                       deps=z))
        red, removed = w.redundant, 0
        for step in range(2):
            red = (_split_on_keys(_with(w, red=red), step, hist) if step == 0 else
                   synth.merge_redundant(red, 5, "span", hist_hlc=hist, step_frac=0.4))
            removed += p.merge(red)["n_keys"][0]
            for scan in A.RECOVER_SCANS:
                got = p.st.recovery_scan(w.queries, scan)
                exp = p.orc.recovery_batch(w.queries, scan)
                ok, why = got.equals(exp, detail=True)
                assert ok, (step, scan, why)
        assert removed > 0
    finally:
        p.close()


def test_advance_keeps_host_lists_across_dictionary_merge(oracle):
    # ad_redundant_advance with host-held missing() lists and watermarks older than the dictionary's newest id: the
    # dictionary merges (ranks move, entries do not), the lists stay aligned -- recovery scans go on answering
    w = synth.recovery_workload(6550, n_redundant=6)
    hist = int(synth._hlc(w.cfk.txn).max())
    p = Pair(w)
    try:
        red = w.redundant
        for step in range(2):
            red = synth.advance_redundant(red, 40 + step, step_frac=0.2, hist_hlc=hist, frac=1.0)
            newest = max(w.cfk.txn.tuples() + w.queries.txn.tuples(), key=lambda t: (t[0], t[1] >> 16))
            assert all((t[0], t[1] >> 16) < (newest[0], newest[1] >> 16) for t in red.wm.tuples())
            stats = p.st.redundant_advance(red)
            assert stats["n_keys"][2] > 0
            p.orc.redundant_advance(red)
            for scan in A.RECOVER_SCANS:
                got = p.st.recovery_scan(w.queries, scan)
                ok, why = got.equals(p.orc.recovery_batch(w.queries, scan), detail=True)
                assert ok, (step, scan, why)
    finally:
        p.close()


@pytest.mark.parametrize("path", [0, 1])
def test_config2_successive_merges(oracle, path):
    # a split, a split of a split, a join and a watermark-only move, with one ad_cfk_update batch and one
    # ad_range_cmds_update in between; config 2 holds no missing() lists, so a fresh oracle store with the
    # current state is the reference of every step. ms_ingest reports the last build: unchanged = no rebuild.
    import cfk_update as U
    import cfk_update_gen as G
    import refmodel
    w = synth.with_redundant_ranges(synth.config2(n_txns=20000, n_keys=20000, n_hist_entries=200000), 16, seed=3)
    hist = int(synth._hlc(w.cfk.txn).max())
    nk = len(w.cfk.keys)
    st = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices, path=path)
    try:
        st.load(w)
        got = st.calculate_partial_deps(w.queries, w.flags)
        assert got.equals(oracle.resolve(w))
        ingest = got.stats["ms_ingest"]
        assert ingest > 0
        red, cfk, cmds, removed = w.redundant, w.cfk, w.cmds, 0
        width = (red.range_end - red.range_start).tolist()
        big = int(np.argmax(width))
        s, e = int(red.range_start[big]), int(red.range_end[big])
        q = (e - s) // 8
        steps = [dict(ranges=[(s + q, s + 5 * q)]), dict(ranges=[(s + 2 * q, s + 3 * q)]), dict(mode="join"),
                 dict(mode="wm", entry=0)]
        for i, kw in enumerate(steps):
            red = synth.merge_redundant(red, 30 + i, hist_hlc=hist, step_frac=0.2, **kw)
            stats = st.redundant_merge(red)
            removed += stats["n_keys"][0]
            if "ranges" in kw:
                assert 0 < stats["n_probes"] < nk and stats["ms_stage"][1] > 0
            if i == 0:
                u = G.fresh_preaccepts(cfk, np.random.default_rng(5), 200, epoch=9)
                cfk, _ = U.cfk_update(cfk, u)
                st.cfk_update(u)
            if i == 1:
                lo, hi = int(cfk.keys.min()), int(cfk.keys.max())
                u = synth.range_cmd_updates(cmds, 8, 20, lo=lo, hi=hi, hlc_hi=900, max_width=(hi - lo) // 50)
                cmds = refmodel.range_cmds_update(cmds, u)
                st.range_cmds_update(u)
            got = st.calculate_partial_deps(w.queries, w.flags)
            ok, why = got.equals(oracle.resolve(_with(w, red=red, cfk=cfk, cmds=cmds)), detail=True)
            assert ok, (i, why)
            assert got.stats["ms_ingest"] == ingest, "a snapshot build ran"
        assert removed > 0
    finally:
        st.close()


@pytest.mark.parametrize("path", [0, 1])
def test_dictionary_merge_without_removals(oracle, path):
    # new watermarks older than the dictionary's newest id but below every entry, with a boundary change: the
    # dictionary merges (every stored rank moves), nothing is truncated
    w = synth.with_redundant_ranges(synth.config2(n_txns=4000, n_keys=4000, n_hist_entries=40000), 12, seed=4,
                                    none_frac=1.0)
    st = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices, path=path)
    try:
        st.load(w)
        assert st.calculate_partial_deps(w.queries, w.flags).equals(oracle.resolve(w))
        lo, hi = int(w.cfk.keys.min()) - 1, int(w.cfk.keys.max()) + 1
        red = synth.merge_redundant(w.redundant, 1, "split", hlc=0)
        red = synth.merge_redundant(red, 2, "gap", hlc=0, lo=lo, hi=hi)
        stats = st.redundant_merge(red)
        n_ids = len({e[4] for e in red.entries() if e[4] != (0, 0, 0)})
        assert stats["n_keys"][0] == 0 and stats["n_keys"][2] == n_ids > 0 and stats["ms_stage"][1] > 0
        got = st.calculate_partial_deps(w.queries, w.flags)
        ok, why = got.equals(oracle.resolve(_with(w, red=red)), detail=True)
        assert ok, why
    finally:
        st.close()


def _store_views(st):
    keys, seg, txn, pruned = st.cfk_byid()
    s, x = st.cfk_entries()
    off, m = st.cfk_missing()
    return (keys.tolist(), seg.tolist(), txn.tuples(), pruned.tolist(), s.tolist(), x.tuples(), off.tolist(), m.tuples())


def test_unchanged_boundaries_equal_advance(oracle):
    w = synth.recovery_workload(6600, n_redundant=6)
    hist = int(synth._hlc(w.cfk.txn).max())
    red = synth.advance_redundant(w.redundant, 7, step_frac=0.4, hist_hlc=hist, frac=0.7)
    a = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices)
    b = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices)
    try:
        a.load(w)
        b.load(w)
        sa, sb = a.redundant_advance(red), b.redundant_merge(red)
        assert sa["n_keys"] == sb["n_keys"] and sa["n_keys"][0] > 0
        assert sb["ms_stage"][1] == 0 and sb["n_probes"] == len(w.cfk.keys)
        assert _store_views(a) == _store_views(b)
        w2 = _with(w, red=red)
        ga, gb = a.calculate_partial_deps(w.queries, w.flags), b.calculate_partial_deps(w.queries, w.flags)
        assert ga.equals(gb) and gb.equals(oracle.resolve(w2))
    finally:
        a.close()
        b.close()


def test_merge_errors(oracle):
    w = _small(6700, n_redundant=6)
    red = w.redundant
    ents = red.entries()
    live = [i for i, e in enumerate(ents) if e[4] != (0, 0, 0)]
    i = max(live, key=lambda j: ents[j][1] - ents[j][0])
    s, e, e0, e1, wm = ents[i]
    assert e - s >= 3
    none = (0, 0, 0)
    back = ents[:i] + [(s, s + 1, e0, e1, wm), (s + 1, e, e0, e1, none)] + ents[i + 1:]     # a piece falls back
    dropped = ents[:i] + [(s, s + 1, e0, e1, wm)] + ents[i + 1:]                            # coverage lost over wm
    overlap = ents[:i] + [(s, e - 1, e0, e1, wm), (e - 2, e, e0, e1, wm)] + ents[i + 1:]
    unsorted_ = ents[::-1] if len(ents) > 1 else ents
    key_dom = ents[:i] + [(s, e, e0, e1, (wm[0], wm[1] & ~1, wm[2]))] + ents[i + 1:]
    st = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices)
    try:
        st.load(w)
        before = st.calculate_partial_deps(w.queries, w.flags)
        v0 = _store_views(st)
        for name, bad in (("back", back), ("dropped", dropped), ("overlap", overlap), ("unsorted", unsorted_),
                          ("key-domain", key_dom)):
            with pytest.raises(native.AccordDepsError) as err:
                st.redundant_merge(Redundant.from_entries(bad))
            assert err.value.code == A.AD_E_INVAL, name
            assert "ad_redundant_merge" in str(err.value), name
        # the store answers exactly as before
        assert st.calculate_partial_deps(w.queries, w.flags).equals(before)
        assert _store_views(st) == v0
        assert before.equals(oracle.resolve(w))
    finally:
        st.close()


def test_before_first_build(oracle):
    # after the load, before any batch: the same as loading the merged map
    w = _small(6800, n_redundant=5, truncated=False)
    hist = int(synth._hlc(w.cfk.txn).max())
    red = synth.merge_redundant(w.redundant, 4, "split", hist_hlc=hist, step_frac=0.5)
    st = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices)
    try:
        st.load(w, prepare=False)
        stats = st.redundant_merge(red)
        assert stats["ms_device"] == 0 and stats["n_probes"] == 0
        got = st.calculate_partial_deps(w.queries, w.flags)
        w2 = _with(w, red=red)
        assert got.equals(oracle.resolve(w2)) and got.equals(native.resolve(w2))
    finally:
        st.close()
