"""Pin of the oracle by random closed-loop Oxford + Primitive episodes that the LIVE reference played
(tests/golden/live_oxford_*.npz, written by `tests/golden/make_golden.py live ...`): each is replayed through the oracle's
restatement of the step, the planner and the gaze policy -- gaze action, plan() result, head waypoint, len(trajectory) and
the full state of every step."""
import pytest

from test_plugins_cpu import _closed_loop

N_EPISODES = 8
SEED = 4242           # make_golden.py live <dir> 4242 8


def _trace(seed):
    return f'live_oxford_{seed}'


@pytest.mark.parametrize('k', range(N_EPISODES))
def test_oracle_reproduces_live_reference_episode(pkg, oracle, k):
    _closed_loop(pkg, oracle, _trace(SEED + k))


N_WIDE = 6
SEED_WIDE = 9100      # make_golden.py live <dir> 9100 6 wide: map sizes, drone radius / acceleration limit / yaw rate, short views,
#                       a target next to the start


@pytest.mark.parametrize('k', range(N_WIDE))
def test_oracle_reproduces_live_reference_episode_wide(pkg, oracle, k):
    _closed_loop(pkg, oracle, _trace(SEED_WIDE + k))
