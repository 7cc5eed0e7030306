#!/usr/bin/env python3
"""Wall-clock cost of the traversability and survival-fit tables (metrics.traversibility_table, metrics.survival_fit_table,
DESIGN.md section 3.11): the reference's traversibility.csv, 20 map_ids x 27 settings = 540 worlds x 81 starts x 8 directions in
three batches (one per agent count), and its metrics_fit.csv, 800 settings of map 0 x 64 positions x 120 checks in ten batches.

Per run and per batch the seconds of metrics.traversibility_batch / survival_fit_batch(timings=...): building the worlds
(`build_s`: on the host one after the other, or on the device), the launch (`launch_s`), the copy of its integers to the host
(`d2h_s`) and the host post-processing into the reference's floats (`post_s`), each with a device synchronise on both sides.  One
small table of each kind is computed untimed first (code objects, allocator); then the runs alternate between worlds='device' and
host worlds.  Every run is kept, not a best-of.  The reference's own seconds per env_metrics(index) call are those the recorder
measured when it wrote tests/golden/difficulty_tables.npz (one world each, on the recording machine's CPU); the tables' fixture
entries are checked against the recorded means on the way.

python tools/difficulty_bench.py --out profiles/difficulty_tables.json"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ('build_s', 'launch_s', 'd2h_s', 'post_s')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--maps', type=int, default=20, help='map_ids 0 .. maps - 1 of the traversability table (the published table: 20)')
    ap.add_argument('--bench-lines', nargs='*', default=[], help='label=file pairs: bench.py result lines taken in the same call, kept in the output')
    ap.add_argument('--out', help='write the result here (JSON)')
    args = ap.parse_args()
    import numpy as np
    import torch
    import drone2d_amd  # noqa: F401
    from drone2d_amd import _lib, metrics, sweeps
    hip = _lib.HipBackend()
    tables = {
        'traversibility': (metrics.traversibility_table, dict(map_ids=range(args.maps)), dict(map_ids=range(1)),
                           sweeps._table_order(range(args.maps), (10, 20, 30), (5, 10, 15), (20, 40, 60)), 'traversibility', 'trav_ref_seconds'),
        'survival_fit': (metrics.survival_fit_table, dict(), dict(agent_numbers=(10, 28), agent_sizes=(5,), agent_speeds=(20,)),
                         sweeps._table_order([0], range(10, 30, 2), range(5, 15), range(20, 60, 5)), 'fit', 'fit_ref_seconds'),
    }
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'difficulty_tables.npz'))
    result = dict(tool='tools/difficulty_bench.py', reps=args.reps, device=torch.cuda.get_device_name(0), tables={})
    for name, (fn, kw, warm, order, key, sec) in tables.items():
        fn(backend=hip, **warm)
        fn(backend=hip, worlds='device', **warm)
        runs, table = [], None
        for rep in range(args.reps):
            for worlds in ('device', None):
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn(backend=hip, worlds=worlds, timings=tm, **kw)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                assert table is None or got == table
                table = got
                rec = dict(rep=rep, worlds='device' if worlds else 'host', n_worlds=tm['worlds'], total_s=total, **{k: tm[k] for k in PARTS},
                           batches=tm['batches'])
                runs.append(rec)
                print(json.dumps(dict(table=name, **{k: v for k, v in rec.items() if k != 'batches'})), flush=True)
        flat = [v for row in table for v in row]
        assert len(flat) == len(order)
        ref = []
        for i in range(int(z['n'])):
            index = json.loads(str(z[f's{i}_index']))
            k = order.index(index) if index in order else None
            same = None if k is None else bool(float(flat[k]).hex() == float(z[f's{i}_{key}']).hex())
            assert same is not False, (name, index)
            ref.append(dict(index=index, reference_seconds=float(z[f's{i}_{sec}']), value=float(z[f's{i}_{key}']), table_entry_equal=same))
        result['tables'][name] = dict(settings=len(order), reference=ref, runs=runs)
    result['bench_lines'] = {}
    for pair in args.bench_lines:
        label, path = pair.split('=', 1)
        lines = [ln for ln in open(path).read().splitlines() if ln.startswith('{')]
        result['bench_lines'][label] = json.loads(lines[-1]) if lines else None
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()
