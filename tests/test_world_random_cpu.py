"""The sequential host form of the device world construction (csrc/worlds/d2d_worlds.h, built by tests/csrc/world_host.c) on the
random worlds of world_random.py against host_init.init_world, every field bit for bit; the conditions that keep that soak (and
the GPU one of test_gpu_device_worlds.py, which runs the same batches) from going quiet, computed from the reference's own call
counts; and the boundary of d2d_world_spec.max_attempts, which host_init does not have."""
import numpy as np
import pytest

import world_cases as WC
import world_random as WR
from rng_host import needs_fma, needs_glibc_235


@pytest.fixture(scope='module')
def host(tmp_path_factory):
    return WC.build_world_host(tmp_path_factory.mktemp('worldhost_random'))


def _with_rng(plist):
    return any(p.var_cam != 0 for p in plist)


def test_counting_random_builds_the_same_world(pkg):
    from drone2d_amd import host_init
    from drone2d_amd.params import with_defaults
    plist, _ = next(WR.batches(WR.SEED, 1))
    for p in plist + [WR.cap_world(1, 0)[0]]:
        plain, (counted, c) = host_init.init_world(with_defaults(p)), WR.counted_world(p)
        assert plain.keys() == counted.keys()
        for k in plain:
            assert np.array_equal(plain[k], counted[k]), k
        assert c['agent_attempts'] >= p.agent_number and c['rounds'] >= p.pillar_number
        assert c['pillar_words'] == 3 * c['rounds'] + c['redraws']


def test_carry_sizes_model():
    assert WR.carry_sizes(0, 0) == [] and WR.carry_sizes(0, 1) == [0] and WR.carry_sizes(0, 104) == [0]
    assert WR.carry_sizes(0, 105) == [0, 0] and WR.carry_sizes(3, 1) == [] and WR.carry_sizes(3, 103) == []
    assert WR.carry_sizes(3, 104) == [3] and WR.carry_sizes(624 + 19, 400) == [5, 5, 5]
    assert WR.carry_sizes(620, 2) == [4] and WR.carry_sizes(624, 1) == [0]


def test_no_world_is_left_out_and_the_soak_covers_the_kernels_paths():
    """On the committed seed, from the reference's counts alone: every batch is 8 built worlds, and among them are the cases the
    device algorithm treats differently from the sequential one."""
    ref = WR.reference()
    assert len(ref) == WR.COUNT and all(len(plist) == WR.ENVS == len(counts) for plist, _, _, counts in ref)
    worlds = [(p, opts, c) for plist, opts, _, counts in ref for p, c in zip(plist, counts)]
    assert len(worlds) == 480
    carries = set()
    for _, _, c in worlds:
        carries.update(WR.carry_sizes(c['pillar_words'], c['agent_attempts']))
    assert carries == {0, 1, 2, 3, 4, 5}
    assert sum(c['agent_attempts'] > 312 for _, _, c in worlds) >= 5            # three or more regenerations
    assert sum(c['rounds'] > p.pillar_number for p, _, c in worlds) >= 5       # a pillar candidate refused
    assert sum(c['redraws'] > 0 for _, _, c in worlds) >= 5
    # a first pass from an empty list: these rejections are the in-pass re-test's on the device
    assert sum(p.agent_number >= 33 and p.pillar_number == 0 and c['agent_attempts'] - p.agent_number >= 5 for p, _, c in worlds) >= 10
    assert {p.agent_number for p, _, _ in worlds} == set(WR.AGENT_NUMBERS)
    odd = {opts['grid_tile'] for p, opts, _ in worlds if p.pillar_number > 0 and
           ((p.map_size[0] // p.map_scale) % 16 or (p.map_size[1] // p.map_scale) % 16)}
    assert odd == {0, 16}
    # what the case table never had: grids whose bytes per env are no multiple of 4, scales other than 10, fractional radii
    assert any((p.map_size[0] // p.map_scale) * (p.map_size[1] // p.map_scale) % 4 and not opts['grid_tile'] for p, opts, _ in worlds)
    assert {p.map_scale for p, _, _ in worlds} == {5, 10, 20} and any(p.agent_radius == 7.5 for p, _, _ in worlds)
    assert any(_with_rng([p]) for p, _, _ in worlds) and not all(_with_rng([p]) for p, _, _ in worlds)


@needs_glibc_235
@needs_fma
def test_random_soak(pkg, host):
    for k, (plist, opts, exp, _) in enumerate(WR.reference()):
        got = host[1](pkg, plist, grid_tile=opts['grid_tile'], rng=_with_rng(plist))
        try:
            WC.assert_equal(got, exp, _with_rng(plist))
        except AssertionError as e:
            raise AssertionError(f'batch {k}: {vars(plist[0])} {opts}') from e
        assert np.array_equal(got['group'], exp['group'])


@needs_glibc_235
@needs_fma
@pytest.mark.parametrize('cfg', range(len(WR.CAP_CONFIGS)))
def test_cap_boundary(pkg, host, cfg):
    """a world that takes A attempts builds with max_attempts = A and is refused with A - 1"""
    for map_id in range(4):
        p, exp, A = WR.cap_world(cfg, map_id)
        assert A >= 2
        WC.assert_equal(host[1](pkg, [p], max_attempts=A), exp, False)
        WC.assert_capped(host[1](pkg, [p], max_attempts=A - 1))


@needs_glibc_235
@needs_fma
@pytest.mark.parametrize('cfg', WR.CAP_MIXED, ids=lambda c: f"n{c['agent_number']}")
def test_cap_mixes_built_and_refused_envs(pkg, host, cfg):
    plist, exp, A, cap = WR.cap_mixed(cfg)
    got = host[1](pkg, plist, max_attempts=cap)
    built = np.array([a <= cap for a in A])
    assert np.array_equal(got['status'], (~built).astype(np.int32))
    WC.assert_equal(WR.env_slice(got, built), WR.env_slice(exp, built), False)
    WC.assert_capped(WR.env_slice(got, ~built))
