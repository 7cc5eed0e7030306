"""d2d_jerk_plan_live of libd2d_jerk.so (include/d2d_jerk_live.h) on the device (run with -m gpu): on the synthetic batches of
tests/jerk_cases.py, 15 envs each (two of every kind and one more), a live env gets bit for bit what d2d_jerk_plan gives it and what
the Python model says, and of a finished env none of the seven buffers the launch writes is touched.  The batches: no trackers
(NULL tracker pointers), three, 70 (two tracker passes) on a 37 x 45 tiled grid (partial edge tiles), and v_max = 4, whose 90 samples a
primitive take the kernel's walk for S > 64."""
import numpy as np
import pytest
import torch

from drone2d_amd import _abi as A
import jerk_cases as JC
import jerk_model as M

pytestmark = pytest.mark.gpu
B = 15
BATCHES = [(0, 40, 50, 50, 0), (3, 20, 50, 50, 0), (70, 40, 37, 45, 16), (3, 4, 37, 45, 16)]
DONE = {'none': np.zeros(B, bool), 'all': np.ones(B, bool), 'every_second': np.arange(B) % 2 == 1, 'last': np.arange(B) == B - 1}
WRITTEN = ('plan_ok', 'wp_valid', 'wp', 'choice', 'stat', 'trk_radius', 'trk_prev')
OTHER_RADIUS, OTHER_PREV = 1234.5, 9          # recognisable: no batch holds them


def upload(arr, dev):
    return {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in arr.items()}


def download(t):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in t.items()}


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope='module')
def unmasked(hip):
    """d2d_jerk_plan on every batch, once: what a live env has to get"""
    out = {}
    for N, v_max, W, H, tile in BATCHES:
        b = JC.batch(B, N, v_max, W, H, tile)
        t = upload(JC.host_arrays(b), hip.device)
        hip.jerk_plan(JC.call_of(b, lambda x: x.data_ptr(), t))
        hip.sync()
        out[N, v_max, W, H, tile] = download(t)
    return out


def test_the_batches_are_what_the_cases_need():
    assert [JC.tables(v)[2] for v in (40, 20, 4)] == [9, 18, 90] and 64 < 90 <= A.JERK_MAX_S
    kinds = JC.batch(B, 3, 20, 50, 50, 0)['kinds']
    assert all(kinds.count(k) >= 2 for k in JC.KINDS) and len(kinds) == B == 2 * len(JC.KINDS) + 1
    arch = np.array(kinds) == 'archived'
    assert (arch & DONE['every_second']).any() and (arch & ~DONE['every_second']).any()
    for N, v_max, W, H, tile in BATCHES:
        if N:       # an archived env whose radius goes back to agent_radius is live under one pattern and finished under another:
            b = JC.batch(B, N, v_max, W, H, tile)                       # the write-back is seen happening and not happening
            back = arch & (b['radius_after'] != b['radius0']).any(1) & (b['prev_after'] != b['prev']).any(1)
            assert any((back & ~d).any() for d in DONE.values()) and any((back & d).any() for d in DONE.values()), (N, v_max)
            if (N, v_max) != (3, 20):                                   # (there env 6's radii were agent_radius already)
                assert (back & ~DONE['every_second']).any() and (back & DONE['every_second']).any()    # ... within one launch


@pytest.mark.parametrize('own_start', [True, False], ids=['own_start', 'other_values_in_finished_rows'])
@pytest.mark.parametrize('done', list(DONE), ids=list(DONE))
@pytest.mark.parametrize('N,v_max,W,H,tile', BATCHES, ids=lambda v: str(v))
def test_live_envs_get_the_plan_and_finished_envs_keep_everything(hip, unmasked, N, v_max, W, H, tile, done, own_start):
    b, want = JC.batch(B, N, v_max, W, H, tile), JC.answers(B, N, v_max, W, H, tile)
    fin = DONE[done]
    arr = JC.host_arrays(b)                                            # the five outputs poisoned
    if N and not own_start:
        arr['trk_radius'][fin], arr['trk_prev'][fin] = OTHER_RADIUS, OTHER_PREV
    before = {k: None if arr[k] is None else arr[k].copy() for k in WRITTEN}
    flags = np.full((B, 4), 1, np.uint8)                               # the other three bytes of an env are not looked at
    flags[:, A.JERK_LIVE_F_DONE] = fin
    flags[fin & (np.arange(B) % 4 == 1), A.JERK_LIVE_F_DONE] = 255     # any non-zero byte says done
    t = upload(arr, hip.device)
    hip.jerk_plan_live(JC.call_of(b, lambda x: x.data_ptr(), t), torch.from_numpy(flags).to(hip.device))
    hip.sync()
    got, ref = download(t), unmasked[N, v_max, W, H, tile]
    for k in WRITTEN:
        if got[k] is None:
            assert N == 0 and k in ('trk_radius', 'trk_prev')
            continue
        assert same(got[k][fin], before[k][fin]), k                    # a finished env: exactly what it was before the launch
        assert same(got[k][~fin], ref[k][~fin]), k                     # a live env: d2d_jerk_plan, bit for bit
    for k in arr:
        if k not in WRITTEN and arr[k] is not None:
            assert same(got[k], arr[k]), k                             # the inputs are inputs
    # ... and the model
    live = ~fin
    assert not want['unknown'].any()
    assert np.array_equal(got['plan_ok'][live], want['plan_ok'][live]) and np.array_equal(got['wp_valid'][live], want['plan_ok'][live])
    assert np.array_equal(got['choice'][live], want['choice'][live]) and M.bits_equal(got['wp'][live], want['wp'][live])
    assert np.array_equal((got['stat'][live] & A.JERK_STAT_TIE) != 0, want['tie'][live])
    assert not (got['stat'][live] & A.JERK_STAT_UNKNOWN).any()
    assert np.array_equal(got['stat'][live] >> A.JERK_STAT_SHIFT, want['tested'][live])
    if N:
        assert M.bits_equal(got['trk_radius'][live], b['radius_after'][live]) and np.array_equal(got['trk_prev'][live], b['prev_after'][live])


def test_without_flags_and_above_the_limits_the_launch_is_refused(hip):
    from drone2d_amd import _lib
    b = JC.batch(B, 0, 40, 50, 50, 0)
    t = upload(JC.host_arrays(b), hip.device)
    flags = torch.zeros((B, 4), dtype=torch.uint8, device=hip.device)
    call = JC.call_of(b, lambda x: x.data_ptr(), t)
    with pytest.raises(_lib.D2DError) as e:
        hip.jerk_plan_live(call, None)
    assert str(e.value) == 'd2d_jerk error -1: d2d_jerk_plan_live: flags is NULL (d2d_jerk_plan is the launch without a mask)'
    call.S = A.JERK_MAX_S + 1
    with pytest.raises(_lib.D2DError, match='-4') as e:
        hip.jerk_plan_live(call, flags)
    with pytest.raises(_lib.D2DError, match='-4') as f:
        hip.jerk_plan(call)
    assert str(e.value).replace('d2d_jerk_plan_live:', 'd2d_jerk_plan:') == str(f.value) and 'samples a primitive' in str(f.value)
    call = JC.call_of(b, lambda x: x.data_ptr(), t)
    call.N = A.JERK_MAX_N + 1
    with pytest.raises(_lib.D2DError, match='-4') as e:
        hip.jerk_plan_live(call, flags)
    with pytest.raises(_lib.D2DError, match='-4') as f:
        hip.jerk_plan(call)
    assert str(e.value).replace('d2d_jerk_plan_live:', 'd2d_jerk_plan:') == str(f.value) and 'trackers' in str(f.value)
    hip.sync()
    assert hip.supports_jerk_live is True
