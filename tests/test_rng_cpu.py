"""csrc/d2d_rng.h (MT19937 + numpy's legacy Gaussian: the stream the reference draws its measurement noise from, utils.py:603-605)
compiled for the host, against np.random.RandomState draw for draw; and the stream state host_init.init_world hands over."""
import numpy as np
import pytest

from rng_host import RNG_NPAIR, RNG_NREGEN, RNG_POS, assert_state_is, build_rng_host, needs_fma, needs_glibc_235, numpy_pairs, numpy_stream

SEEDS = (0, 1, 2, 3, 7, 1234, 4242, 9104, 2 ** 31 - 1)
BATCHES = (0, 1, 3, 64, 65, 172)


@pytest.fixture(scope='module')
def rng_draw(tmp_path_factory):
    return build_rng_host(tmp_path_factory.mktemp('rng'))


def _world_rng(pkg, seed):
    from drone2d_amd import host_init
    p = pkg.with_defaults(pkg.Params(planner='NoMove', agent_number=3, agent_radius=10, map_id=seed))
    return host_init.init_world(p)['rng']


@pytest.mark.parametrize('seed', SEEDS)
def test_init_world_returns_the_reference_stream(pkg, seed):
    """np.random.seed(map_id) and the 100 rand() of the static-map velocities (envs/drone_v2.py:80, :51-55): position 200, the key
    of the seed, an empty Gaussian cache -- read from the constructing stream itself, not assumed"""
    rng = _world_rng(pkg, seed)
    assert rng.dtype == np.uint32 and rng.shape == (pkg._abi.RNG_WORDS,)
    ref = np.random.RandomState(seed)
    ref.rand(100)
    assert int(rng[RNG_POS]) == 200
    assert_state_is(rng, ref)


@needs_glibc_235
@needs_fma
@pytest.mark.parametrize('seed', SEEDS)
def test_host_stream_equals_numpy_draw_for_draw(pkg, rng_draw, seed):
    state = _world_rng(pkg, seed).copy()
    ref = numpy_stream(state)
    order = np.random.RandomState(seed ^ 0x5bd1).permutation(np.repeat(BATCHES, 7))    # 42 batches, 2135 pairs, uneven sizes
    drawn = 0
    for i, m in enumerate(order):
        got = rng_draw(state, int(m))
        want = numpy_pairs(ref, int(m))
        assert got.tobytes() == want.tobytes(), (seed, i, m)
        drawn += int(m)
        assert_state_is(state, ref, (seed, i, m))
        assert int(state[RNG_NPAIR]) == drawn
    assert drawn >= 2000 and int(state[RNG_NREGEN]) >= 10


@needs_glibc_235
@needs_fma
def test_host_stream_from_an_unaligned_position(rng_draw):
    """a state whose position is no multiple of 4 (an attempt then straddles the end of the key): the host path still follows numpy"""
    ref = np.random.RandomState(11)
    ref.rand(3)                                          # position 6
    ref.randint(0, 10, 1)                                # one more word: 7
    _, key, pos, _, _ = ref.get_state()
    assert pos % 4 != 0
    state = np.zeros(640, dtype=np.uint32)
    state[:624], state[RNG_POS] = key, pos
    for m in (5, 170, 1, 300):
        assert rng_draw(state, m).tobytes() == numpy_pairs(ref, m).tobytes()
        assert_state_is(state, ref, m)


def test_unaligned_streams_are_refused_before_upload(pkg):
    from drone2d_amd import state
    rng = np.zeros((2, pkg._abi.RNG_WORDS), dtype=np.uint32)
    rng[:, RNG_POS] = (200, 624)
    state.check_rng(rng)
    for bad in (201, 625, 2 ** 31):
        rng[1, RNG_POS] = bad
        with pytest.raises(ValueError, match='multiples of 4'):
            state.check_rng(rng)


def test_a_backend_without_the_stage_sees_no_stream(pkg, oracle):
    """var_cam != 0 on the oracle: the state holds the streams, the structs the backend gets do not -- it goes on taking the draws
    as an input (set_noise), as before; worlds that do not carry a stream (built by hand) allocate none"""
    from drone2d_amd import vec_env
    p = pkg.Params(var_cam=2, planner='NoMove', agent_number=10, agent_radius=15, map_id=1)
    env = vec_env.VecDrone2DEnv(p, 2, backend=oracle)
    assert not env.device_noise and not env._st.rng and not env._st.rng_draws and not env._init_st.rng
    assert int(env.state.rng[1, RNG_POS]) == 200 and env.init_state.rng is not env.state.rng
    worlds = [{k: v for k, v in w.items() if k != 'rng'} for w in vec_env.build_worlds(p, 2)]
    bare = vec_env.VecDrone2DEnv(p, 2, backend=oracle, worlds=worlds)
    assert 'rng' not in bare.state.t and not bare.device_noise
    quiet = vec_env.VecDrone2DEnv(pkg.Params(planner='NoMove', agent_number=10, agent_radius=15, map_id=1), 2, backend=oracle)
    assert 'rng' not in quiet.state.t and not quiet._st.rng                      # var_cam == 0: nothing allocated
