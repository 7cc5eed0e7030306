#!/usr/bin/env python3
"""hidden_dyn_collect.py <out dir of tools/hidden_dyn_bench.sh> <parent libd2d_hip.so> [--alt-lib FILE] [--pmc-before FILE]
> profiles/hidden_dyn.json

Condenses the calls of tools/hidden_dyn_bench.sh into one record, with the pieces of tools/hidden_obs_collect.py: every bench run of both
libraries, the medians, the gain and the parent's range per line, the head of chain_prof, the k_closed rows of the kernel traces, the
static ISA figures of every k_closed instantiation, and the PMC figures per env-step of the config-2 closed loop before (--pmc-before:
the parent's profiles/pmc_latest.json) and after (this tree's).  PARTS=forms runs, if the directory holds them, go under `forms` with
the ISA figures of --alt-lib (the form that was not chosen)."""
import argparse
import csv
import json
import os
import statistics as st
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hidden_obs_collect as H
import isa_stats as I


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('parent_lib')
    ap.add_argument('--alt-lib')
    ap.add_argument('--pmc-before')
    a = ap.parse_args()
    d = a.out
    res = {'note': 'One MI355X, tools/hidden_dyn_bench.sh: every command alternated between the parent commit\'s library and this tree\'s '
                   '(D2D_LIB).  bench_* values are env-steps/s of bench.py\'s closed loop (600_300 and 20_5: config 2, 4096 envs, '
                   'k_closed<1, true>; config3 / config4 / config5: --workload, window / tile kernels that this change leaves on the '
                   'every-step stage); closed_65536 = tools/closed_loop_bench.py --envs 65536 --streams 1; chain_prof = the '
                   '-DD2D_CHAIN_PROF builds; kernel_trace = the k_closed dispatches of `rocprofv3 --kernel-trace --stats` over the '
                   '600 / 300 command, a pass of its own; pmc = profiles/pmc_latest.json of the parent commit and of this tree; forms = '
                   'the 600 / 300 line with the library of the other form (a second instantiation of run_env) as a third alternative.  '
                   'The bar of the change: the 600 / 300 gain above twice the parent\'s range (gain_exceeds_twice_parent_range).',
           'runs': {}, 'summary': {}}
    for name in ('bench_600_300', 'bench_20_5', 'bench_config3', 'bench_config4', 'bench_config5', 'closed_65536'):
        p, t = H.runs(d, name, 'parent'), H.runs(d, name, 'this')
        if p and t:
            res['runs'][name] = {'parent': p, 'this': t}
            res['summary'][name] = H.summary(p, t)
            s = res['summary'][name]
            s['gain_exceeds_twice_parent_range'] = bool(s['gain_pct'] > 2 * s['parent_range_pct'])
    forms = {w: H.runs(d, 'forms_600_300', w) for w in ('parent', 'this', 'alt')}
    if all(forms.values()):
        res['forms'] = {'runs': forms, 'this_vs_parent': H.summary(forms['parent'], forms['this']),
                        'alt_vs_parent': H.summary(forms['parent'], forms['alt'])}
    for which in ('parent', 'this'):
        f = os.path.join(d, f'chain_prof_{which}.out')
        if os.path.exists(f):
            res.setdefault('chain_prof', {})[which] = open(f).read().splitlines()[:14]
        f = os.path.join(d, f'kernel_trace_closed_{which}.csv')
        if os.path.exists(f):
            kc = [r for r in csv.DictReader(open(f)) if 'k_closed<' in r['Kernel_Name']]
            res.setdefault('kernel_trace', {})[which] = dict(
                kernel=sorted({I.short_name(r['Kernel_Name']).replace('void ', '') for r in kc}),
                launches_us=[round((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3, 1) for r in kc],
                vgpr_count=sorted({int(r['VGPR_Count']) for r in kc}), scratch_size=sorted({int(r['Scratch_Size']) for r in kc}))
    if 'kernel_trace' in res:
        res['summary']['kernel_trace_mean_us'] = {k: round(st.mean(v['launches_us']), 1) for k, v in res['kernel_trace'].items()}
    res['isa'] = {'parent': H.isa(a.parent_lib), 'this': H.isa(H.THIS)}
    if a.alt_lib:
        res['isa']['alt'] = H.isa(a.alt_lib)
    if a.pmc_before:
        b, t = H.pmc(a.pmc_before), H.pmc(os.path.join(H.ROOT, 'profiles', 'pmc_latest.json'))
        res['pmc_per_env_step'] = {'before': b, 'after': t, 'drop': {k: round(b[k] - t[k], 1) for k in H.PMC_KEYS if k in b and k in t}}
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
