"""tests/jerk_model.py, the Jerk_Primitive planner in this project's own words, against the recorded reference
(tests/golden/jerk_traces.npz), and the tie table (drone2d_amd.jerk_plugin.tie_table) against numpy's live argsort."""
import numpy as np
import pytest

from drone2d_amd import _abi as A
from drone2d_amd import jerk_plugin as JP
import jerk_env_cases as EC
import jerk_model as M


@pytest.mark.parametrize('i', range(len(EC.world_names())), ids=EC.world_names())
def test_model_reproduces_every_recorded_step(pkg, i):
    """choice, wp, plan_ok, phi_h bit for bit, walking the headings in the RECORDED numpy's order (the fixture's tie table) so that
    a host whose argsort breaks ties another way still checks the arithmetic; where the table does not describe a step's costs the
    model's own argsort is used and the step is counted"""
    w = EC.world(i)
    perm, eq = EC.tie_table()
    off_table = 0
    for t in range(len(w['t_done'])):
        sc = EC.scene(pkg, w, t)
        phi = M.goal_direction(sc)
        cost = M.costs(phi)
        pat = JP.pattern_of(phi)
        fits = JP.table_fits(perm[pat], eq[pat], cost)
        off_table += not fits
        r = M.plan(sc, order=perm[pat].astype(np.int64) if fits else None)
        assert M.bits_equal(r['phi_h'], w['t_phi_h'][t]), t
        assert r['plan_ok'] == w['t_plan_ok'][t] and r['choice'] == w['t_choice'][t], t
        assert M.bits_equal(r['wp'], w['t_wp'][t]), t
        assert r['tie'] == bool(w['t_tie'][t]), t
    assert off_table == 0


def test_recorded_worlds_cover_what_they_are_for():
    names = EC.world_names()
    assert {'default40', 'default20', 'obstacle_map', 'var_cam2', 'two_targets', 'rvo'} <= set(names)
    w = {n: EC.world(i) for i, n in enumerate(names)}
    assert (w['default20']['t_plan_ok'] == 0).any() and w['default20']['t_fail'].max() >= 1          # failing plans, the brake
    assert len(set(w['obstacle_map']['t_choice'].tolist())) >= 5                                       # walls reject headings
    assert len({tuple(t) for t in w['two_targets']['t_p_target']}) == 2
    assert any(x['t_p_active'].any() for x in w.values())
    assert np.abs(w['two_targets']['t_vel'][:, 2:]).max() > 0                                          # the acceleration is written
    if 'tie' in w:
        assert w['tie']['t_tie'].any()


def test_tie_table_of_this_host_equals_the_recorded_one_under_the_same_numpy():
    z = EC.traces()
    perm, eq = JP.tie_table()
    assert perm.shape == eq.shape == (A.JERK_PATTERNS, A.JERK_NTHETA) and perm.dtype == eq.dtype == np.uint8
    assert np.array_equal(eq, z['tie_eq'])                  # the weak orders themselves do not depend on numpy
    assert eq[0::4].sum(axis=1).tolist() == [35] * 72 and eq[2::4].sum(axis=1).tolist() == [36] * 72
    assert not eq[1::4].any() and not eq[3::4].any()
    if str(z['numpy_version']) != np.__version__:
        pytest.skip(f"recorded under numpy {z['numpy_version']}, this is {np.__version__}: the order inside tied pairs may differ")
    assert np.array_equal(perm, z['tie_perm'])


def test_table_rule_holds_for_random_goal_directions():
    """200 phi per pattern: wherever the row of the phi's pattern fits the costs, it IS numpy's live argsort; rows that do not fit
    are counted (none: random phi are never within 1e-13 degrees of a multiple of 2.5)"""
    perm, eq = JP.tie_table()
    rng = np.random.RandomState(72)
    misfit = 0
    for pat in range(A.JERK_PATTERNS):
        k, kind = divmod(pat, 4)
        if kind in (0, 2):
            offs = np.full(200, 0.0 if kind == 0 else 2.5)
            turns = rng.randint(-3, 4, 200) * 360.0                    # the same direction, other representations of phi
        else:
            offs = rng.uniform(0.0, 2.5, 200) + (0.0 if kind == 1 else 2.5)
            turns = np.zeros(200)
        for off, turn in zip(offs, turns):
            phi = 5.0 * k + off + turn
            if kind in (1, 3) and (off % 2.5 == 0.0):
                continue
            cost = JP.heading_costs(phi)
            p = JP.pattern_of(phi)
            if not JP.table_fits(perm[p], eq[p], cost):
                misfit += 1
                continue
            assert p == pat or kind in (1, 3)
            assert np.array_equal(np.argsort(cost), perm[p]), (pat, phi)
    assert misfit == 0


def test_an_inconsistent_argsort_is_refused():
    calls = [0]

    def flaky(c):
        calls[0] += 1
        order = np.argsort(c, kind='stable')
        return order[::-1] if calls[0] % 2 == 0 else order
    with pytest.raises(RuntimeError, match='tie table'):
        JP.tie_table(argsort=flaky)


def test_primitive_tables_are_the_model_s_numbers():
    for v_max, S in ((7, 51), (20, 18), (40, 9), (72, 5)):
        th, tt, s = JP.primitive_tables(v_max, 0.1)
        assert s == S == tt.shape[1] and th.shape == (72, 8) and int(th[:, 7].max()) == S
        sc = dict(drone=(100.0, 100.0, 0.0, 0.0, 0.0, 0.0), target=(300.0, 300.0), v_max=v_max, dt=0.1)
        for i in (0, 1, 17, 18, 35, 71):
            ts = M.primitive(sc, 5.0 * i)[3]
            assert len(ts) == int(th[i, 7]) and M.bits_equal(tt[i, :len(ts), 0], ts)
            assert M.bits_equal(tt[i, :len(ts), 4], [x ** 5 for x in ts])
    assert {int(x) for x in JP.primitive_tables(20, 0.1)[0][:, 7]} == {17, 18}
    with pytest.raises(ValueError, match='at most 128'):
        JP.primitive_tables(2, 0.1)
