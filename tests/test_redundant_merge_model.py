"""model.Redundant.merge (RedundantBefore.merge, RedundantBefore.java:375-377: ReducingIntervalMap.mergeIntervals
with Entry.merge :121-157, Builder.slice :473-479, tryMergeEqual :488-498) against a pointwise model written here:
at every point of the key line the merged map holds exactly Entry.merge of what the two inputs hold there."""
import numpy as np
import pytest

from accord_deps import _abi as A
from accord_deps import synth
from accord_deps.model import Redundant, make_txn_ids


def _order(t):
    return (t[0], t[1] >> 16, t[1] & 0x1E, t[2])          # Timestamp.compareTo (Timestamp.java:208-217)


def _wm(hlc, node=1, epoch=1):
    return make_txn_ids(epoch, np.array([hlc], np.uint64), A.KIND_EXCLUSIVE_SYNC_POINT, node, domain=1).tuples()[0]


NONE = (0, 0, 0)


def _holding(ents, x, incl):
    """(startEpoch, endEpoch, wm) of the entry holding point x (Range.contains in the inclusivity), or None."""
    for s, e, e0, e1, wm in ents:
        if (s <= x < e) if incl else (s < x <= e):
            return (e0, e1, wm)
    return None


def _entry_merge(a, b):
    """Entry.merge (RedundantBefore.java:121-157) of two holders of one point (None: no entry)."""
    if a is None or b is None:
        return a if b is None else b
    if a[0] > b[1]:
        return a
    if b[0] > a[1]:
        return b
    return (max(a[0], b[0]), min(a[1], b[1]), a[2] if _order(a[2]) >= _order(b[2]) else b[2])


def _points(*maps):
    """every integer key of [-530, 530] and both sides of every boundary (half-integers stand for the open side)"""
    pts = set(range(-530, 531))
    for m in maps:
        for s, e in zip(m.range_start.tolist(), m.range_end.tolist()):
            pts.update((s - 0.5, s, s + 0.5, e - 0.5, e, e + 0.5))
    return sorted(pts)


def _check(a, b):
    m = Redundant.merge(a, b)
    ea, eb, em = a.entries(), b.entries(), m.entries()
    for i, (s, e, e0, e1, wm) in enumerate(em):
        assert s < e, (i, s, e)
        if i:
            assert em[i - 1][1] <= s, "entries ascending and disjoint"
            assert not (em[i - 1][1] == s and em[i - 1][2:] == (e0, e1, wm)), "touching equal entries are joined"
    for incl in (False, True):
        for x in _points(a, b, m):
            exp = _entry_merge(_holding(ea, x, incl), _holding(eb, x, incl))
            assert _holding(em, x, incl) == exp, (incl, x)
    return m


def _random_map(rng, n):
    pts = np.sort(rng.choice(np.arange(-520, 520), 2 * n, replace=False)).tolist()
    if n > 1 and rng.random() < 0.5:                     # some touching entries
        j = int(rng.integers(0, n - 1))
        pts[2 * j + 1] = pts[2 * j + 2]
    ents = []
    for i in range(n):
        wm = NONE if rng.random() < 0.2 else _wm(int(rng.integers(1, 8)), int(rng.integers(1, 3)), int(rng.integers(1, 3)))
        e0 = int(rng.integers(0, 4))
        ents.append((pts[2 * i], pts[2 * i + 1], e0, e0 + int(rng.integers(0, 4)), wm))
    return Redundant.from_entries(ents)


@pytest.mark.parametrize("seed", range(200))
def test_random_pairs(seed):
    rng = np.random.default_rng(9000 + seed)
    _check(_random_map(rng, int(rng.integers(0, 7))), _random_map(rng, int(rng.integers(0, 7))))


def test_split_into_three():
    a = Redundant.from_entries([(0, 100, 1, 9, _wm(5))])
    m = _check(a, Redundant.from_entries([(40, 60, 1, 9, _wm(8))]))
    assert m.entries() == [(0, 40, 1, 9, _wm(5)), (40, 60, 1, 9, _wm(8)), (60, 100, 1, 9, _wm(5))]


def test_join():
    a = Redundant.from_entries([(0, 40, 1, 9, _wm(5)), (40, 60, 1, 9, _wm(8)), (60, 100, 1, 9, _wm(5))])
    m = _check(a, Redundant.from_entries([(0, 40, 1, 9, _wm(8)), (60, 100, 1, 9, _wm(8))]))
    assert m.entries() == [(0, 100, 1, 9, _wm(8))]
    # equal watermarks, other epochs: kept apart
    m = _check(a, Redundant.from_entries([(0, 40, 2, 9, _wm(8))]))
    assert [e[:2] for e in m.entries()] == [(0, 40), (40, 60), (60, 100)]


def test_gap_fill():
    a = Redundant.from_entries([(0, 10, 1, 9, _wm(5)), (30, 40, 1, 9, _wm(5))])
    m = _check(a, Redundant.from_entries([(10, 30, 1, 9, _wm(5))]))
    assert m.entries() == [(0, 40, 1, 9, _wm(5))]
    m = _check(a, Redundant.from_entries([(12, 20, 1, 9, _wm(7))]))
    assert [e[:2] for e in m.entries()] == [(0, 10), (12, 20), (30, 40)]


def test_epoch_disjoint_keeps_one_side():
    a = Redundant.from_entries([(0, 100, 5, 9, _wm(5))])
    b = Redundant.from_entries([(20, 50, 1, 4, _wm(8))])
    assert _check(a, b).entries() == a.entries()                          # a.startEpoch > b.endEpoch: keep a
    m = _check(b, a)                                                      # b.startEpoch > a.endEpoch: keep b (= a here)
    assert m.entries() == a.entries()
    b2 = Redundant.from_entries([(20, 50, 10, 12, _wm(3))])
    assert _check(a, b2).entries() == [(0, 20, 5, 9, _wm(5)), (20, 50, 10, 12, _wm(3)), (50, 100, 5, 9, _wm(5))]


def test_empty_side():
    a = Redundant.from_entries([(0, 10, 1, 9, _wm(5)), (10, 20, 1, 9, NONE)])
    assert _check(a, Redundant.empty()).entries() == a.entries()
    assert _check(Redundant.empty(), a).entries() == a.entries()
    assert len(_check(Redundant.empty(), Redundant.empty()).range_start) == 0


@pytest.mark.parametrize("mode", ["split", "gap", "wm", "span", "join"])
@pytest.mark.parametrize("seed", range(6))
def test_synth_merge_redundant_moves_forward(seed, mode):
    # the generator's additions never let the effective watermark of a point fall back
    red = synth.random_small(9300 + seed, n_redundant=3 + seed % 5).redundant
    if mode == "join":
        red = synth.merge_redundant(red, seed, "split")              # a split's pieces touch
    new, add = synth.merge_redundant(red, 50 + seed, mode, return_add=True)
    assert 1 <= len(add.range_start) <= 3
    eo, en = red.entries(), new.entries()
    for x in _points(red, new):
        o, n_ = _holding(eo, x, False), _holding(en, x, False)
        assert _order((n_ or (0, 0, NONE))[2]) >= _order((o or (0, 0, NONE))[2]), x
    if mode == "split":
        assert len(en) == len(eo) + 2
    if mode == "join":
        assert len(en) == len(eo) - 1
    if mode == "wm":
        assert [e[:2] for e in en] == [e[:2] for e in eo]
    if mode == "span" and len({e[2:4] for e in eo}) == 1:
        assert len(en) == 1
