#!/usr/bin/env python3
"""plan_fold_collect.py <out dir of tools/plan_fold_bench.sh> <parent libd2d_hip.so> [options] > profiles/plan_fold.json

Condenses one call of tools/plan_fold_bench.sh: every bench run of both libraries, the medians, the parent's range and standard
deviation, search_bench's lone failing search, the head of chain_prof, the k_closed rows of the kernel traces, and the static ISA figures
(tools/isa_stats.py) of k_closed<1> in the parent's library and of k_closed<1, false> / k_closed<1, true> in this tree's.
  --diag PARENT.so THIS.so   the -DD2D_CHAIN_PROF -DD2D_SEARCH_PROF builds of both trees: their kernels cut at the clock stamps
                             (isa_stats.regions), with --cell-loop P T and --expansion P0:P1 T0:T1 naming the pieces that are the gaze
                             stage's per-cell pass and the search's expansion loop
  --variant NAME DIR         a further call of the script with another library in the parent's place (its bench runs only)"""
import argparse
import csv
import json
import os
import re
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_stats as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THIS = os.path.join(ROOT, 'gym-drone2d-activeperception_amd', 'csrc', 'libd2d_hip.so')


def bench_runs(d, kind, which):
    out = []
    for i in range(1, 100):
        f = os.path.join(d, f'bench_{kind}_{which}_{i}.out')
        if not os.path.exists(f):
            break
        out.append(json.loads(open(f).read().strip().splitlines()[-1])['value'])
    return out


def summary(parent, this):
    pm, tm = st.median(parent), st.median(this)
    gain, rng = (tm / pm - 1) * 100, (max(parent) - min(parent)) / pm * 100
    return dict(parent_median=pm, this_median=tm, gain_pct=round(gain, 2), parent_range_pct=round(rng, 2),
                parent_stdev_pct=round(st.stdev(parent) / pm * 100, 2), this_range_pct=round((max(this) - min(this)) / tm * 100, 2),
                gain_exceeds_parent_range=bool(gain > rng))


def isa(lib, names):
    funcs, meta = I.collect(lib)
    by_name = {I.short_name(k).replace('void ', ''): v for k, v in funcs.items()}
    regs = {I.demangle(k).replace('void ', ''): v for k, v in meta.items()}
    out = {}
    for n in names:
        c, m = by_name[n], regs[n]
        valu = sum(c[k] for k in I.VALU_CLASSES)
        scalar = c['salu'] + c['s_load'] + c['s_wait'] + c['s_branch']
        out[n] = dict(instructions=c['_total'], valu=valu, salu=c['salu'], s_load=c['s_load'], s_waitcnt=c['s_wait'], s_branch=c['s_branch'],
                      scalar_share=round(scalar / c['_total'], 3), lds=c['lds'], vmem=c['vmem'], scratch_instructions=c['scratch'],
                      vgpr=int(m['vgpr_count']), sgpr=int(m['sgpr_count']), sgpr_spill=int(m['sgpr_spill_count']),
                      vgpr_spill=int(m['vgpr_spill_count']), scratch_bytes=int(m['private_segment_fixed_size']))
    return out


def pieces(lib, kernel):
    return [dict(instructions=c['_total'], s_load=c['s_load'], s_branch=c['s_branch'], salu=c['salu'], s_waitcnt=c['s_wait'])
            for c in I.regions(lib, kernel)]


def span(ps, a, b):
    return {k: sum(p[k] for p in ps[a:b + 1]) for k in ('instructions', 's_load', 's_branch', 'salu', 's_waitcnt')}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('parent_lib')
    ap.add_argument('--diag', nargs=2)
    ap.add_argument('--cell-loop', nargs=2, type=int)
    ap.add_argument('--expansion', nargs=2)
    ap.add_argument('--variant', nargs=2, action='append', default=[])
    a = ap.parse_args()
    d = a.out
    res = {'note': 'One MI355X, one call of tools/plan_fold_bench.sh: every command alternated between the parent commit\'s library and this '
                   'tree\'s (D2D_LIB).  bench values are env-steps/s of the config-2 closed loop (4096 envs, k_closed); search_bench = '
                   'tools/search_bench.py --envs 1 (k_plan, which this change does not touch: a control); chain_prof = the '
                   '-DD2D_CHAIN_PROF builds; kernel_trace = the k_closed dispatches of `rocprofv3 --kernel-trace --stats` over the 600 / 300 '
                   'command, a pass of its own.'}
    for kind in ('600_300', '20_5'):
        for which in ('parent', 'this'):
            res[f'bench_{kind}' + ('_parent' if which == 'parent' else '')] = bench_runs(d, kind, which)
    res['summary'] = {f'bench_{k}': summary(res[f'bench_{k}_parent'], res[f'bench_{k}']) for k in ('600_300', '20_5')}
    for which in ('parent', 'this'):
        txt = open(os.path.join(d, f'search_bench_{which}.out')).read()
        m = re.search(r'deadlock_primitive B=1: (.*?) \|', txt)
        res.setdefault('search_bench_lone_failing_search_us', {})[which] = [int(x.split('us')[0]) for x in m.group(1).split()]
        res.setdefault('chain_prof', {})[which] = open(os.path.join(d, f'chain_prof_{which}.out')).read().splitlines()[:14]
        rows = list(csv.DictReader(open(os.path.join(d, f'kernel_trace_closed_{which}.csv'))))
        kc = [r for r in rows if 'k_closed<' in r['Kernel_Name']]
        res.setdefault('kernel_trace', {})[which] = dict(
            kernel=sorted({I.short_name(r['Kernel_Name']).replace('void ', '') for r in kc}),
            launches_us=[round((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3, 1) for r in kc],
            vgpr_count=sorted({int(r['VGPR_Count']) for r in kc}), scratch_size=sorted({int(r['Scratch_Size']) for r in kc}))
        res.setdefault('kernel_stats', {})[which] = [ln for ln in open(os.path.join(d, f'kernel_stats_{which}.csv')).read().splitlines()[:6]]
    sb = res['search_bench_lone_failing_search_us']
    res['summary']['search_bench_lone_median_us'] = {k: st.median(v[1:]) for k, v in sb.items()}      # (the first launch is the cold one)
    kt = res['kernel_trace']
    res['summary']['kernel_trace_mean_us'] = {k: round(st.mean(v['launches_us']), 1) for k, v in kt.items()}
    res['isa'] = {'parent': isa(a.parent_lib, ['k_closed<1>']), 'this': isa(THIS, ['k_closed<1, false>', 'k_closed<1, true>'])}
    if a.diag:
        pp, tp = pieces(a.diag[0], 'k_closed<1>'), pieces(a.diag[1], 'k_closed<1, true>')
        sec = {'note': 'the kernels of the -DD2D_CHAIN_PROF -DD2D_SEARCH_PROF builds cut at their clock stamps, in address order '
                       '(tools/isa_stats.py regions): static counts per piece, roughly per stamped section',
               'parent_pieces': pp, 'this_pieces': tp}
        if a.cell_loop:
            sec['gaze_per_cell_pass'] = {'parent': pp[a.cell_loop[0]], 'this': tp[a.cell_loop[1]]}
        if a.expansion:
            (p0, p1), (t0, t1) = (tuple(int(x) for x in s.split(':')) for s in a.expansion)
            sec['search_expansion_loop'] = {'parent': span(pp, p0, p1), 'this': span(tp, t0, t1)}
        res['isa_sections'] = sec
    for name, vd in a.variant:
        v = {k: bench_runs(vd, k, 'parent') for k in ('600_300', '20_5')}
        t = {k: bench_runs(vd, k, 'this') for k in ('600_300', '20_5')}
        res.setdefault('variants', {})[name] = {
            'note': 'a further call of the script with this library in the parent\'s place: its own runs of this tree\'s library beside it',
            **{f'bench_{k}_{name}': v[k] for k in v}, **{f'bench_{k}_this': t[k] for k in t},
            'summary': {f'bench_{k}': summary(v[k], t[k]) for k in v}}
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
