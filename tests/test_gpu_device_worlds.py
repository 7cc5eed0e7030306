"""The seeded worlds built on the device (include/d2d_worlds.h, csrc/worlds/) against host_init.init_world: the case table of
world_cases.py field by field, then the env, the survivability table and the experiment batch on device-built worlds against the
same objects on host-built worlds; then the random worlds of world_random.py (the batches whose coverage test_world_random_cpu.py
asserts), a poisoned and fenced destination, the boundary of max_attempts and a launch of 1024 workgroups.  Every comparison is
exact."""
import copy

import numpy as np
import pytest
import torch

import world_cases as WC
import world_random as WR

pytestmark = pytest.mark.gpu


def _device_fields(dw):
    out = {f: dw.state.t[f].cpu().numpy() for f in WC.FIELDS}
    if 'rng' in dw.state.t:
        out['rng'] = dw.state.t['rng'].cpu().numpy()
    out.update(tracker_radius=dw.tracker_radius.numpy(), obstacles=dw.obstacles, status=dw.status)
    return out


@pytest.mark.parametrize('name', WC.CASE_NAMES)
def test_case_table(pkg, hip, name):
    from drone2d_amd import vec_env, _lib
    plist, opt = WC.cases(pkg)[name]
    tile = opt.get('grid_tile', 0)
    layout = 'tiled' if tile else 'rowmajor'
    if opt.get('capped'):
        with pytest.raises(_lib.D2DError, match=r'env 0 \(map_id 0\)'):
            vec_env.build_worlds_device_of(plist, backend=hip, max_attempts=opt['max_attempts'])
        dw = vec_env.build_worlds_device_of(plist, backend=hip, max_attempts=opt['max_attempts'], check=False)
        WC.assert_capped(_device_fields(dw))
        return
    if name == 'three_targets_offset5':        # the sharding offset: map_id 0 + env_offset 5 + i
        p = copy.copy(plist[0])
        p.map_id = 0
        dw = vec_env.build_worlds_device(p, len(plist), env_offset=5, backend=hip, grid_layout=layout)
    else:
        dw = vec_env.build_worlds_device_of(plist, backend=hip, grid_layout=layout)
    exp = WC.expected(pkg, name, plist, tile)
    with_rng = any(p.var_cam != 0 for p in plist)
    assert with_rng == ('rng' in dw.state.t)
    WC.assert_equal(_device_fields(dw), exp, with_rng)
    assert np.array_equal(dw.group, exp['group']) and (dw.N, dw.T) == (exp['agents'].shape[2], exp['targets'].shape[1])


def _same_state(a, b, plugins=False):
    assert set(a.state.t) == set(b.state.t)
    for name in a.state.t:
        assert torch.equal(a.state.t[name].cpu(), b.state.t[name].cpu()), name
    for name in ('agents', 'gt', 'dmap', 'drone', 'counters', 'kf', 'kf_len', 'active'):
        assert torch.equal(a.init_state.t[name].cpu(), b.init_state.t[name].cpu()), 'snapshot ' + name
    assert torch.equal(a.tracker_radius, b.tracker_radius)
    if plugins:
        assert torch.equal(a.plugins.t['traj_hdr'].cpu(), b.plugins.t['traj_hdr'].cpu())


def test_env_on_device_worlds_steps_like_host_worlds(pkg, hip):
    from drone2d_amd import vec_env
    p = pkg.Params(planner='NoMove', agent_number=10, agent_radius=15, agent_max_speed=20, map_id=1, var_cam=2)
    host = vec_env.VecDrone2DEnv(p, 8, backend=hip)
    dev = vec_env.VecDrone2DEnv(p, 8, backend=hip, worlds='device')
    _same_state(host, dev)
    rng = np.random.RandomState(0)
    for _ in range(10):
        a = rng.uniform(-1, 1, 8)
        host.step(a)
        dev.step(a)
    host.sync()
    _same_state(host, dev)


def test_closed_loop_with_auto_reset_on_device_worlds(pkg, hip):
    from drone2d_amd import vec_env
    q = pkg.Params(planner='Primitive', gaze_method='Oxford', agent_number=10, agent_radius=15, agent_max_speed=20,
                   drone_max_speed=40, map_id=1)
    kw = dict(backend=hip, planner='Primitive', device_plugins=True, gaze='Oxford')
    host = vec_env.VecDrone2DEnv(q, 6, **kw)
    dev = vec_env.VecDrone2DEnv(q, 6, worlds=vec_env.build_worlds_device(q, 6, backend=hip), **kw)
    host.closed_loop(40, auto_reset=True)
    dev.closed_loop(40, auto_reset=True)
    host.sync()
    _same_state(host, dev, plugins=True)


def test_survivability_table_on_device_worlds(pkg, hip):
    from drone2d_amd import sweeps
    host = sweeps.survivability_table(map_ids=[0], backend=hip)
    dev = sweeps.survivability_table(map_ids=[0], backend=hip, worlds='device')
    assert host.shape == dev.shape and np.array_equal(host, dev)


def test_experiment_batch_on_device_worlds(pkg, hip):
    from drone2d_amd import runner
    p = pkg.Params(planner='Primitive', gaze_method='Oxford', agent_number=10, agent_radius=15, agent_max_speed=20,
                   drone_max_speed=40, map_id=3, max_flight_time=6)
    host = runner.ExperimentBatch(p, 6, backend=hip)
    dev = runner.ExperimentBatch(p, 6, backend=hip, device_worlds=True)
    rows_h, rows_d = host.run(), dev.run()
    assert len(rows_d) == 6 and [tuple(map(str, r)) for r in rows_h] == [tuple(map(str, r)) for r in rows_d]


# ---------------------------------------------------------------------------------------- random worlds, poison, cap, many workgroups
def _with_rng(plist):
    return any(p.var_cam != 0 for p in plist)


def test_random_soak(pkg, hip):
    """the 60 batches of world_random.py: odd grids in both layouts, scales 5 / 10 / 20, fractional radii, per-env rows that differ
    inside a launch, every carry size, worlds of three and more regenerations"""
    from drone2d_amd import vec_env
    for k, (plist, opts, exp, _) in enumerate(WR.reference()):
        dw = vec_env.build_worlds_device_of(plist, backend=hip, grid_layout='tiled' if opts['grid_tile'] else 'rowmajor')
        assert _with_rng(plist) == ('rng' in dw.state.t)
        try:
            WC.assert_equal(_device_fields(dw), exp, _with_rng(plist))
        except AssertionError as e:
            raise AssertionError(f'batch {k}: {vars(plist[0])} {opts}') from e
        assert np.array_equal(dw.group, exp['group'])


FENCE, POISON, GUARD = 256, 0x77, 0xA5
POISON_CASES = {
    # name: (per-batch Params, grid_tile, byte offsets of gt and dmap from a 4-byte boundary)
    'odd_rowmajor': (dict(map_size=[250, 250], pillar_number=3, agent_number=7, init_pos=[60, 60], target_list=[[200, 200]]), 0, (0, 1, 2, 3)),
    'random_map_0_rng': (dict(map_size=[480, 640], static_map='maps/random_map_0.npy', var_cam=2, agent_number=10), 0, (0,)),
    'odd_tiled': (dict(map_size=[330, 270], pillar_number=1, agent_number=33, init_pos=[60, 60], target_list=[[280, 220]]), 16, (0,)),
}


@pytest.mark.parametrize('name,shift', [(n, s) for n, c in POISON_CASES.items() for s in c[2]])
def test_poisoned_and_fenced_destination(pkg, hip, name, shift):
    """Every world field is a view into a larger buffer: 0x77 where the kernel must write, 0xA5 on 256 bytes either side.  The
    kernel must leave no byte of a field unwritten (BatchState presets kf and kf_len and zero-fills the rest, which would hide
    that) and none of a fence touched.  A 25 x 25 row-major grid is 625 B per env, so envs 1, 2 and 3 start at the three
    misalignments of fill_bytes; `shift` moves env 0 there as well.  tracker_radius, obstacles and status are allocated inside
    _build_into and stay unfenced."""
    from drone2d_amd import host_init, state, vec_env
    kw, tile, _ = POISON_CASES[name]
    plist = [pkg.Params(planner='NoMove', map_id=m, agent_radius=r, agent_max_speed=v, **kw)
             for m, r, v in zip(range(3, 11), (5, 7.5, 10, 12, -1, 5, 10, 7.5), (20, 33.3, 40, 60) * 2)]
    inp = vec_env.world_inputs(plist)
    p0 = pkg.with_defaults(plist[0])
    st = state.BatchState(host_init.derive_cfg(p0, B=inp['U'], N=inp['N'], T=inp['T'], grid_tile=tile), hip.device)
    assert (st.cfg.W * st.cfg.H % 4 != 0) == name.startswith('odd')
    raws = {}
    for f in state.WORLD_FIELDS + ('rng_draws',):
        if f not in st.t:
            continue
        t = st.t[f]
        nbytes = t.numel() * t.element_size()
        start = FENCE + (shift if f in ('gt', 'dmap') else 0)
        raw = torch.full((start + nbytes + FENCE,), GUARD, dtype=torch.uint8, device=hip.device)
        assert nbytes > 0 and raw.data_ptr() % 8 == 0
        raw[start:start + nbytes] = POISON
        st.t[f] = raw[start:start + nbytes].view(t.dtype).view(t.shape)
        assert st.t[f].data_ptr() == raw.data_ptr() + start
        raws[f] = (raw, start, nbytes)
    tr, obs, status = vec_env._build_into(hip, inp, st)
    got = {f: st.t[f].cpu().numpy() for f in WC.FIELDS}
    with_rng = _with_rng(plist)
    assert with_rng == ('rng' in st.t)
    if with_rng:
        got['rng'] = st.t['rng'].cpu().numpy()
        assert not got['rng'][:, 625:].any() and not st.t['rng_draws'].cpu().numpy().any()
    got.update(tracker_radius=tr.numpy(), obstacles=obs, status=status)
    exp = WC.expected(pkg, 'poison_' + name, plist, tile)
    WC.assert_equal(got, exp, with_rng)
    for f, (raw, start, nbytes) in raws.items():
        host = raw.cpu().numpy()
        assert (host[:start] == GUARD).all() and (host[start + nbytes:] == GUARD).all(), f'{f}: fence overwritten'
        if f in exp:            # a byte still 0x77 where the reference has another value was never written
            want = np.ascontiguousarray(exp[f]).view(np.uint8).reshape(-1)
            assert want.size == nbytes and not ((host[start:start + nbytes] == POISON) & (want != POISON)).any(), f'{f}: poison left'


@pytest.mark.parametrize('cfg', range(len(WR.CAP_CONFIGS)))
def test_cap_boundary(pkg, hip, cfg):
    """a world that takes A attempts builds with max_attempts = A and is refused with A - 1"""
    from drone2d_amd import vec_env
    for map_id in range(4):
        p, exp, A = WR.cap_world(cfg, map_id)
        WC.assert_equal(_device_fields(vec_env.build_worlds_device_of([p], backend=hip, max_attempts=A)), exp, False)
        WC.assert_capped(_device_fields(vec_env.build_worlds_device_of([p], backend=hip, max_attempts=A - 1, check=False)))


@pytest.mark.parametrize('cfg', WR.CAP_MIXED, ids=lambda c: f"n{c['agent_number']}")
def test_cap_mixes_built_and_refused_envs(pkg, hip, cfg):
    """one launch whose cap is the median A of its 8 envs: with 10 agents the cap shortens the first pass, with 100 and 60 it falls
    behind several passes and a regeneration"""
    from drone2d_amd import vec_env, _lib
    plist, exp, A, cap = WR.cap_mixed(cfg)
    built = np.array([a <= cap for a in A])
    got = _device_fields(vec_env.build_worlds_device_of(plist, backend=hip, max_attempts=cap, check=False))
    assert np.array_equal(got['status'], (~built).astype(np.int32))
    WC.assert_equal(WR.env_slice(got, built), WR.env_slice(exp, built), False)
    WC.assert_capped(WR.env_slice(got, ~built))
    first = int(np.nonzero(~built)[0][0])
    with pytest.raises(_lib.D2DError, match=rf'env {first} \(map_id {plist[first].map_id}\).*max_attempts = {cap} \({int((~built).sum())} of 8 envs\)'):
        vec_env.build_worlds_device_of(plist, backend=hip, max_attempts=cap)


def test_1024_workgroups_up_to_the_last_seed(pkg, hip):
    from drone2d_amd import vec_env
    p = pkg.Params(planner='NoMove', agent_number=10, agent_radius=15, agent_max_speed=20)
    off = 2 ** 32 - 1 - 1023
    dw = vec_env.build_worlds_device(p, 1024, env_offset=off, backend=hip)
    assert dw.map_ids[-1] == 2 ** 32 - 1
    plist = [pkg.Params(planner='NoMove', agent_number=10, agent_radius=15, agent_max_speed=20, map_id=off + i) for i in range(1024)]
    WC.assert_equal(_device_fields(dw), WC.expected(pkg, 'last_1024_seeds', plist), False)
