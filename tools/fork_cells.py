#!/usr/bin/env python3
"""fork_cells.py : chooses the map ids of the slot-fork twin cells (tests/fork_cases.py) on the CPU stand-ins.  For every cell and
every base map id 0, 4, .. 60 an env of 4 slots (map_id + 0 .. 3) plays N0 + N1 steps under the test's seeded actions; a slot is a
witness when it has run a plan search before step N0, has an active tracker at step N0 and ends its episode after it.  Prints, per
cell, the first base map id with a witness and the witness (slot, active trackers at the fork, the step that ended the episode), or
says that no map id below 64 has one.  A cell the stand-ins cannot step (the device noise stream) is tried with var_cam = 0 worlds'
twin, which moves the same agents: its choice is then confirmed by the GPU test's own assertion."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def witness_of(pkg, cell, map_id):
    import fork_backend as FB
    import fork_cases as FC
    from drone2d_amd import _abi as A
    kw = dict(FC.CELLS[cell][0])
    if FC.CELLS[cell][2]:
        kw.pop('var_cam')
    env = FB.env_of(pkg.Params(map_id=map_id, **kw), FC.B_A, channels='swept_obs' in FC.CELLS[cell][1], **FC.env_kw(cell))
    acts = FC.actions(FC.N0 + FC.N1, FC.B_A)
    ended = [0] * FC.B_A
    for t in range(FC.N0 + FC.N1):
        if t == FC.N0:
            searched, trackers = FC.searched(env).tolist(), env.state.active.sum(1).tolist()
        FC.step(env, acts[t])
        done = env.state.flags[:, A.F_DONE].tolist()
        ended = [ended[i] or (t + 1 if done[i] else 0) for i in range(FC.B_A)]
    return [(i, int(trackers[i]), ended[i]) for i in range(FC.B_A) if searched[i] and trackers[i] > 0 and ended[i] > FC.N0]


def main():
    import drone2d_amd as pkg
    import fork_cases as FC
    for cell in (sys.argv[1:] or FC.CELLS):
        for map_id in range(0, 64, 4):
            w = witness_of(pkg, cell, map_id)
            if w:
                print(f'{cell}: map_id {map_id}: witness (slot, trackers at the fork, ended at step) {w[0]}', flush=True)
                break
        else:
            print(f'{cell}: no map_id below 64 shows a slot that searched, tracks and ends within {FC.N0} + {FC.N1} steps', flush=True)


if __name__ == '__main__':
    main()
