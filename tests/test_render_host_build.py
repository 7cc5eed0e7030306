"""csrc/render/d2d_render.h compiled for the host with gcc under AddressSanitizer and UBSan, as the stand-alone program
tests/csrc/render_host_main.c, run as a child process over buffers that end with their last byte: the digests of its frames are those
of the numpy model (tests/render_model.py) for every handmade case, and its display lists are the model's, byte for byte, for the
states of a replayed episode.  Nothing sanitized is loaded into this process."""
import math
import subprocess

import numpy as np
import pytest
import torch

import host_build
import render_cases as RC

pytestmark = host_build.needs_fma('the host build of csrc/d2d_sincos.h is the FMA variant of libm')


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    return host_build.sanitized(['render_host_main.c'], tmp_path_factory.mktemp('render_host'), 'render_host')


def _run(program, tmp_path, records):
    src, out = tmp_path / 'in.bin', tmp_path / 'out.bin'
    with open(src, 'wb') as f:
        f.write(np.array([len(records)], np.int32).tobytes())
        for r in records:
            f.write(r)
    res = subprocess.run([program, str(src), str(out)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    return out.read_bytes()


def _raster_record(c, cap=None):
    n = int(c['list']['count'])
    cap = max(n, 1) if cap is None else cap
    head = np.array([1, cap, c['W'], c['H'], c['W_px'], c['H_px'], c['scale'], c['d'], n], np.int32)
    return head.tobytes() + RC.to_bytes(c['list'], cap).tobytes() + np.ascontiguousarray(c['cells']).tobytes()


def test_the_handmade_cases_give_the_model_s_digests(program, tmp_path):
    cases = RC.handmade()
    names = [c['name'] for c in cases]
    # what the set is for: the frame's corners, items outside, more items than a pass keeps, the five arc ranges, downsample 1 .. 3,
    # a row pitch that is no multiple of 16
    assert {'corners', 'outside', 'many', 'arcs', 'many-d2', 'arcs-d3', 'pitch-203', 'beyond-the-map'} <= set(names)
    assert int(cases[names.index('many')]['list']['count']) > 128 and (203 * 3) % 16 != 0
    assert sorted(set(cases[names.index('arcs')]['list']['geom'][:, 10].tolist())) == [90.0, 120.0, 180.0, 270.0, 360.0, 400.0]
    out = _run(program, tmp_path, [_raster_record(c) for c in cases])
    got = np.frombuffer(out, dtype=np.uint64)
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        frame = RC.model_frame(c)
        assert frame.shape == (-(-c['H_px'] // c['d']), -(-c['W_px'] // c['d']), 3)
        assert int(g) == RC.digest(frame), c['name']
    # the frames are not trivial: every case but the empty one differs from its cell layer
    import render_model as RM
    for c in cases:
        plain = RM.cell_layer(c['cells'], c['W_px'], c['H_px'], c['scale'], c['d'])
        assert np.array_equal(RC.model_frame(c), plain) == (c['name'] == 'empty'), c['name']


def _list_record(st, cap):
    N, P = st['agents'].shape[1], len(st['pillars'])
    traj = np.zeros((0, 2)) if st['traj'] is None else np.asarray(st['traj'], dtype=np.float64).reshape(-1, 2)
    star = [f(math.pi / 5 * i) for i in range(10) for f in (math.sin, math.cos)]
    head = np.array([2, N, P, len(traj), st['n_seeded'], st['steps'], int(st['vel'] is not None), cap], np.int32)
    parts = [head, np.array([st['R'], st['view_range'], st['drone_radius']]), st['drone'].astype(np.float64), st['agents'].astype(np.float64),
             st['active'].astype(np.uint8)] + ([st['vel'].astype(np.float64)] if st['vel'] is not None else []) + \
        [st['target'].astype(np.float64), np.asarray(st['pillars'], dtype=np.int32), traj, np.array(star)]
    return b''.join(np.ascontiguousarray(a).tobytes() for a in parts)


@pytest.mark.parametrize('i', [0, 1])
def test_the_host_list_is_the_model_s_byte_for_byte(pkg, program, tmp_path, i):
    """episodes (a) and (b) replayed on the CPU oracle (Primitive under CVM and under RVO with pillars): every fifth step's state
    through d2d_render_list_seq with a capacity of exactly its items, and once with one item less (refused, nothing written)"""
    ep = RC.episode(i)
    env, step = RC.oracle_env(pkg, ep)
    states = [RC.slot_state(env, 0)]                      # before the first step: the seeded agents at rest
    for t, a in enumerate(ep['action']):
        step(float(a))
        if t % 5 == 4:
            states.append(RC.slot_state(env, 0))
    import render_model as RM
    want = [RM.make_list(**st) for st in states]
    records = [_list_record(st, int(w['count'])) for st, w in zip(states, want)] + [_list_record(states[-1], int(want[-1]['count']) - 1)]
    out = _run(program, tmp_path, records)
    off = 0
    for w in want:
        n = int(np.frombuffer(out, np.int32, 1, off)[0])
        assert n == int(w['count'])
        got = np.frombuffer(out, np.uint8, n * RC.ITEM_BYTES, off + 4).reshape(n, RC.ITEM_BYTES)
        assert np.array_equal(got, RC.to_bytes(w, n)), np.argwhere(got != RC.to_bytes(w, n))[:4].tolist()
        off += 4 + n * RC.ITEM_BYTES
    assert int(np.frombuffer(out, np.int32, 1, off)[0]) == -1 and off + 4 == len(out)
    assert any(st['traj'] is not None and len(st['traj']) > 1 for st in states)
