"""The seeded worlds built on the device (include/d2d_worlds.h, csrc/worlds/) against host_init.init_world: the case table of
world_cases.py field by field, then the env, the survivability table and the experiment batch on device-built worlds against the
same objects on host-built worlds.  Every comparison is exact."""
import copy

import numpy as np
import pytest
import torch

import world_cases as WC

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
