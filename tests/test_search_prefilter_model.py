"""The argument behind the device A*'s expansion order, on a model of the reference's dict loop (traj_planner.py:197-206).

The reference applies the successors of one expansion to its open / closed dicts one after the other, in generation order.  The device
consults the dict as it stands BEFORE the expansion, drops what it rejects (key closed, or open at no higher cost) -- before any
collision sample is taken -- and then writes, per key, the cheapest survivor (the earliest on ties) without asking the dict again.
During one expansion a closed key stays closed and an open key's cost only goes down, so the three must leave the same dict: the same
keys, costs AND the same successor behind every key (its payload is the node's parent, position, velocity: what a trajectory is
built from), also where several successors of one node share a key (drone speeds below 13.75)."""
import numpy as np
import pytest

OPEN, CLOSED = 1, 2


def apply_in_order(d, succ):
    """traj_planner.py:197-206 literally; d: key -> [state, cost, payload], succ: (key, cost, payload) in generation order"""
    d = {k: list(v) for k, v in d.items()}
    for key, cost, pay in succ:
        if key in d and d[key][0] == CLOSED:       # :198-199
            continue
        if key not in d:                           # :201-202
            d[key] = [OPEN, cost, pay]
        elif d[key][1] > cost:                     # :204-206
            d[key] = [OPEN, cost, pay]
    return d


def prefilter(d, succ):
    """what the pre-expansion dict does not discard"""
    return [(k, c, p) for k, c, p in succ if k not in d or (d[k][0] != CLOSED and d[k][1] > c)]


def device_write(d, survivors):
    """the device's resolution: per key the cheapest survivor, the earliest on ties, written without another look at the dict"""
    d = {k: list(v) for k, v in d.items()}
    best = {}
    for key, cost, pay in survivors:               # (generation order: strict < keeps the earliest)
        if key not in best or cost < best[key][0]:
            best[key] = (cost, pay)
    for key, (cost, pay) in best.items():
        d[key] = [OPEN, cost, pay]
    return d


def _random_case(rng):
    nkeys = int(rng.randint(1, 24))
    d = {}
    for k in range(nkeys):
        if rng.rand() < 0.6:
            # few distinct cost values: ties between a successor and the dict, and between successors, are common
            d[k] = [int(rng.choice([OPEN, CLOSED])), float(rng.randint(0, 6)), ('old', k)]
    succ = [(int(rng.randint(0, nkeys)), float(rng.randint(0, 6)), ('new', i)) for i in range(int(rng.randint(0, 40)))]
    return d, succ


@pytest.mark.parametrize('seed', range(8))
def test_filtering_against_the_dict_before_the_expansion_changes_nothing(seed):
    rng = np.random.RandomState(seed)
    dropped = repeats = 0
    for _ in range(2500):
        d, succ = _random_case(rng)
        want = apply_in_order(d, succ)
        kept = prefilter(d, succ)
        assert apply_in_order(d, kept) == want       # the issue's statement: filter, then apply the survivors
        assert device_write(d, kept) == want         # the device's form of "apply"
        # a successor that some sample would have rejected is simply missing from the stream: any sub-stream behaves the same
        sub = [s for s in succ if rng.rand() < 0.6]
        assert device_write(d, prefilter(d, sub)) == apply_in_order(d, sub)
        dropped += len(succ) - len(kept)
        repeats += len(kept) - len({k for k, _, _ in kept})
    assert dropped > 1000 and repeats > 1000         # the cases did discard successors, and survivors did share keys


def test_a_rejected_successor_would_be_rejected_in_generation_order_too():
    """the two orders differ only in WHEN a successor is dropped: one the earlier dict accepts may still lose to an earlier sibling,
    never the other way round"""
    d = {7: [OPEN, 3.0, 'old'], 8: [CLOSED, 0.0, 'old']}
    succ = [(7, 2.0, 'a'), (7, 2.0, 'b'), (7, 1.0, 'c'), (7, 3.0, 'd'), (8, -1.0, 'e'), (9, 5.0, 'f'), (9, 5.0, 'g')]
    assert [p for _, _, p in prefilter(d, succ)] == ['a', 'b', 'c', 'f', 'g']
    out = device_write(d, prefilter(d, succ))
    assert out == apply_in_order(d, succ) == {7: [OPEN, 1.0, 'c'], 8: [CLOSED, 0.0, 'old'], 9: [OPEN, 5.0, 'f']}
