"""The numpy model of the renderer (tests/render_model.py, written from include/d2d_render.h) against the reference's recorded draw
calls (tests/golden/render_calls.npz) and against the properties the coverage rules state.  No GPU: the episodes are replayed on the
CPU oracle backends."""
import os

import numpy as np
import pytest
import torch

import render_cases as RC
import render_model as RM


def test_the_fixture_covers_what_it_is_for():
    RC.assert_coverage(RC.coverage())
    assert os.path.getsize(RC.PATH) < 200 * 1000
    cfgs = [RC.episode(i)['cfg'] for i in range(RC.EPISODES)]
    assert [(c['planner'], c.get('motion_profile', 'CVM'), c['drone_view_range']) for c in cfgs] == [
        ('Primitive', 'CVM', 90), ('Primitive', 'RVO', 120), ('Jerk_Primitive', 'CVM', 120), ('NoMove', 'CVM', 360)]
    for i in range(RC.EPISODES):
        ep = RC.episode(i)
        steps = ep['frame_step'].tolist()
        T = len(ep['action'])
        assert steps == sorted(set(range(10, T + 1, 10)) | {T}), i


@pytest.mark.parametrize('i', range(RC.EPISODES))
def test_rectangles_alone_are_the_model_s_cell_layer(pkg, i):
    """every recorded frame: the reference's rectangles (scale i, scale j, scale, scale) painted into a canvas equal cell_layer()"""
    ep = RC.episode(i)
    p = RC.params_of(pkg, ep)
    scale, (W_px, H_px) = p.map_scale, p.map_size
    colour = np.array([100, 200, 240], dtype=np.uint8)
    code = np.array([1, 2, 0], dtype=np.uint8)          # a grid code of each colour index
    for cells in ep['cells']:
        canvas = np.zeros((H_px, W_px, 3), dtype=np.uint8)
        for a in range(cells.shape[0]):
            for b in range(cells.shape[1]):
                canvas[scale * b:scale * b + scale, scale * a:scale * a + scale] = colour[cells[a, b]]
        assert np.array_equal(RM.cell_layer(code[cells], W_px, H_px, scale), canvas)
        assert np.array_equal(RM.cell_layer(code[cells], W_px, H_px, scale, 3), canvas[::3, ::3])


@pytest.mark.parametrize('i', range(RC.EPISODES))
def test_the_model_s_list_is_the_reference_s_calls(pkg, i):
    """the four episodes replayed on the CPU oracle: at every recorded step make_list() of the env's state equals the reference's
    calls in order, kind, colour, width and every float64 as bits, and the explored map gives the recorded cell layer"""
    ep = RC.episode(i)
    env, step = RC.oracle_env(pkg, ep)
    f = 0
    for t, a in enumerate(ep['action']):
        step(float(a))
        if f < len(ep['frame_step']) and int(ep['frame_step'][f]) == t + 1:
            RC.assert_list_is(RC.model_list(env, 0), RC.frame_calls(ep, f), (i, f))
            assert np.array_equal(RC.COLOUR_INDEX[RC.dmap_of(env, 0)], ep['cells'][f]), (i, f)
            f += 1
    assert f == len(ep['frame_step']) and bool(env.state.flags[0, 3])


def _mask(items, W=64, H=48, d=1):
    cells = np.full((-(-W // 10), -(-H // 10)), 2, dtype=np.uint8)
    fr = RM.raster(RM.pack(items), cells, W, H, 10, d)
    return (fr != 200).any(axis=2), fr


def test_the_capsule_is_symmetric():
    m, _ = _mask([RM.line((1, 2, 3), 12, 20, 51, 27, 5)])
    assert m.sum() > 150
    # about its centre (31.5, 23.5): pixel (x, y) <-> (63 - x, 47 - y), and under swapped end points
    assert np.array_equal(m, m[::-1, ::-1])
    assert np.array_equal(m, _mask([RM.line((1, 2, 3), 51, 27, 12, 20, 5)])[0])
    # a horizontal capsule of width 4 from (10, 20) to (30, 20): rows 18 .. 22, round caps of radius 2
    h, _ = _mask([RM.line((9, 9, 9), 10, 20, 30, 20, 4)])
    assert h[18:23, 10:31].all() and not h[17].any() and not h[23].any() and h[20, 8] and not h[20, 7] and h[20, 32] and not h[20, 33]
    assert not h[18, 9] and h[19, 9]


def test_a_degenerate_line_is_a_disc():
    for w in (1.0, 2.0, 7.0):
        a, _ = _mask([RM.line((5, 5, 5), 30, 22, 30, 22, w)])
        b, _ = _mask([RM.disc((5, 5, 5), 30, 22, w / 2)])
        assert np.array_equal(a, b) and a[22, 30]


def test_the_360_degree_arc_is_a_ring_and_the_wedges_add_up():
    ring, _ = _mask([RM.arc((7, 7, 7), 32, 24, 20, 123.0, 360, 3)])
    ys, xs = np.mgrid[0:48, 0:64]
    q = (xs - 32.0) ** 2 + (ys - 24.0) ** 2
    assert np.array_equal(ring, (q >= 17.0 ** 2) & (q <= 20.0 ** 2))
    # 90 + 270 degrees around opposite headings cover the ring, and overlap only on the two shared edges
    a, _ = _mask([RM.arc((7, 7, 7), 32, 24, 20, 30.0, 90, 3)])
    b, _ = _mask([RM.arc((7, 7, 7), 32, 24, 20, 210.0, 270, 3)])
    assert np.array_equal(a | b, ring) and (a & b).sum() <= 8 and a.sum() * 2 < b.sum()
    # heading 0 with 180 degrees: the right half.  (The column x == cx is the two edges themselves, and cos(pi / 2) is 6e-17, not 0: it
    # belongs to whichever side the libm's rounding puts it on, and is not asserted)
    half, _ = _mask([RM.arc((7, 7, 7), 32, 24, 20, 0.0, 180, 3)])
    assert np.array_equal(half[:, 33:], ring[:, 33:]) and not half[:, :32].any()
    up, _ = _mask([RM.arc((7, 7, 7), 32, 24, 20, 90.0, 90, 3)])
    assert up[24 - 19, 32] and not up[24 + 19, 32]           # heading 90 degrees looks up the screen


def test_painter_s_order_and_the_polygon():
    red, blue = (255, 0, 0), (0, 0, 255)
    _, fr = _mask([RM.disc(red, 30, 24, 10), RM.disc(blue, 36, 24, 10)])
    assert tuple(fr[24, 33]) == blue and tuple(fr[24, 22]) == red
    _, fr = _mask([RM.disc(blue, 36, 24, 10), RM.disc(red, 30, 24, 10)])
    assert tuple(fr[24, 33]) == red and tuple(fr[24, 45]) == blue
    sq, _ = _mask([RM.poly(red, [(10.5, 10.5), (20.5, 10.5), (20.5, 30.5), (10.5, 30.5)])])
    assert sq.sum() == 10 * 20 and sq[11:31, 11:21].all()
    assert np.array_equal(sq, _mask([RM.poly(red, [(10.5, 30.5), (20.5, 30.5), (20.5, 10.5), (10.5, 10.5)])])[0])    # either winding
    # downsampling is point sampling of the full frame
    items = RC.handmade()[2]['list']
    c = RC.handmade()[2]
    full = RM.raster(items, c['cells'], c['W_px'], c['H_px'], c['scale'], 1)
    for d in (2, 3):
        assert np.array_equal(RM.raster(items, c['cells'], c['W_px'], c['H_px'], c['scale'], d), full[::d, ::d])
