"""GPU parity of the three TxnInfo.missing() list rebuilds run one after the other on one store: an update
batch with deps (k_miss_build), Pruning.maybePrune (k_miss_build over the kept entries), a RedundantBefore
merge that truncates a sub-range (k_trunc_miss) and another update batch with deps. The three share one host
step (cfk_update.hip rebuild_missing_lists) and one set of persistent work buffers; the other tests run each
on a store of its own. After every step the CommandsForKeys (keys, segments, TxnIds, prunedBefore, statuses,
executeAts), every missing() list, the snapshot's invariants and the deps of a resolve are compared, exactly,
with the oracle restatements (oracle/cfk_update.py; synth.truncate_to_redundant for the truncation)."""
import os
import sys

import numpy as np
import pytest

from accord_deps import native, synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import cfk_update as U  # noqa: E402
import cfk_update_gen as G  # noqa: E402

SEEDS = (1, 4)


def _with(w, red, cfk):
    return type(w)(w.name, cfk, w.cmds, red, w.queries, w.flags, w.params, w.range_start_inclusive, w.slices)


def chain(seed):
    """The workload and the oracle's side of the four steps: [(name, input, expected CommandsForKeys,
    RedundantBefore in force, entries the step removed)]."""
    from test_gpu_cfk_missing import _workload, with_deps
    from test_gpu_cfk_prune import _applied_wave
    w = _workload(90 + seed, n_hist_txns=200)
    rng = np.random.default_rng(seed)
    incl = bool(w.range_start_inclusive)
    steps = []
    u = with_deps(w.cfk, _applied_wave(w.cfk, rng, 0.8), rng, keep=0.9, n_new=0)
    cfk, _, _ = U.cfk_update_missing(w.cfk, u, u.dep_off, u.deps)
    steps.append(("update", u, cfk, w.redundant, 0))
    cfk, removed, _ = U.cfk_prune(cfk, None, 1, 0)
    steps.append(("prune", None, cfk, w.redundant, removed))
    # a sub-range of the RedundantBefore entry holding the most keys, from one of its keys to another, raised to
    # the median hlc of the entries left: about half of those keys' entries lie below it
    ents = w.redundant.entries()
    inside = [[int(k) for k in cfk.keys if s < k < e] for s, e, *_ in ents]
    ks = max(inside, key=len)
    red = synth.merge_redundant(w.redundant, seed, ranges=[(ks[len(ks) // 4], ks[(3 * len(ks)) // 4])],
                                hlc=int(np.median(synth._hlc(cfk.txn))))
    n0 = cfk.n_entries
    cfk = synth.truncate_to_redundant(cfk, red, incl)
    steps.append(("merge", red, cfk, red, n0 - cfk.n_entries))
    u = with_deps(cfk, G.concat(G.transitions(cfk, rng, 40)[0],
                                G.fresh_preaccepts(cfk, rng, 10, statuses=(2, 3), epoch=9, hlc0=1001)), rng)
    cfk, _, _ = U.cfk_update_missing(cfk, u, u.dep_off, u.deps)
    steps.append(("update", u, cfk, red, 0))
    return w, steps


@pytest.mark.parametrize("seed", SEEDS)
def test_chain_oracle_removes_entries(seed):
    # the seeds are chosen so that both removing steps remove something (the oracle side alone, no GPU)
    _, steps = chain(seed)
    assert steps[1][4] > 0, "the prune step removes no entry for this seed"
    assert steps[2][4] > 0, "the merge step truncates no entry for this seed"
    assert not U.dup_committed_exec(steps[3][2])


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_update_prune_truncate_update(oracle, seed):
    w, steps = chain(seed)
    st = native.DeviceCommandStore(0, w.range_start_inclusive, 1, w.slices)
    try:
        st.load(w)
        for i, (name, arg, exp, red, removed) in enumerate(steps):
            if name == "update":
                st.cfk_update(arg)
            elif name == "prune":
                got_removed, _ = st.cfk_prune(None, 1, 0)
                assert got_removed == removed > 0
            else:
                stats = st.redundant_merge(arg)
                assert stats["n_keys"][0] == removed > 0
            tag = "step %d (%s)" % (i + 1, name)
            keys, seg, txn, pruned = st.cfk_byid()
            assert keys.tolist() == exp.keys.tolist() and seg.tolist() == exp.seg.tolist(), tag
            assert [U.norm(*x) for x in txn.tuples()] == [U.norm(*x) for x in exp.txn.tuples()], tag
            exp_pb = exp.pruned_before if exp.pruned_before is not None else np.full(len(keys), -1)
            assert pruned.tolist() == exp_pb.tolist(), tag
            s, x = st.cfk_entries()
            assert s.tolist() == exp.status.tolist(), tag
            assert x.msb.tolist() == exp.exec.msb.tolist() and x.lsb.tolist() == exp.exec.lsb.tolist(), tag
            off, ms = st.cfk_missing()
            assert off.tolist() == exp.miss_off.tolist(), tag + ": missing() list sizes differ"
            assert ([U.norm(*m) for m in ms.tuples()] == [U.norm(*m) for m in exp.miss.tuples()]), tag
            assert st.check_snapshot() == (0, None), tag
            w2 = _with(w, red, exp)
            got = st.calculate_partial_deps(w2.queries, w2.flags)
            ok, why = got.equals(oracle.resolve(w2), detail=True)
            assert ok, (tag, why)
    finally:
        st.close()
