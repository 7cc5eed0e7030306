#!/usr/bin/env python3
"""hidden_obs_collect.py <out dir of tools/hidden_obs_bench.sh> <parent libd2d_hip.so> [--pmc-before FILE] [--isa-notes FILE]
> profiles/hidden_obs.json

Condenses one call of tools/hidden_obs_bench.sh (its two parts may have run as calls of their own into the same directory): every
bench run of both libraries, the medians, the gain, the parent's range (max - min) and standard deviation per line, the head of
chain_prof, the k_closed rows of the kernel traces, the static ISA figures (tools/isa_stats.py) of every k_closed instantiation in both
libraries, and the PMC figures per env-step of the config-2 closed loop before (--pmc-before: the parent's profiles/pmc_latest.json)
and after (this tree's).  --isa-notes: a JSON file of findings read off the disassembly by hand, stored under isa.by_hand."""
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
PMC_KEYS = ('fetch_bytes_per_env_step_raw', 'write_bytes_per_env_step', 'hbm_bytes_per_env_step_raw', 'hbm_bytes_per_env_step',
            'valu_insts_per_env_step', 'salu_insts_per_env_step', 'wave_cycles_per_env_step', 'med_us_rocprof')


def bench_value(path):
    last = open(path).read().strip().splitlines()[-1]
    if last.startswith('{'):
        return json.loads(last)['value']
    return float(re.search(r': ([0-9.e+]+) env-steps/s', last).group(1))        # tools/closed_loop_bench.py


def runs(d, name, which):
    out = []
    for i in range(1, 100):
        f = os.path.join(d, f'{name}_{which}_{i}.out')
        if not os.path.exists(f):
            break
        out.append(bench_value(f))
    return out


def summary(parent, this):
    pm, tm = st.median(parent), st.median(this)
    gain, rng = (tm / pm - 1) * 100, (max(parent) - min(parent)) / pm * 100
    return dict(parent_median=pm, this_median=tm, gain_pct=round(gain, 2), parent_range_pct=round(rng, 2),
                parent_stdev_pct=round(st.stdev(parent) / pm * 100, 2), this_range_pct=round((max(this) - min(this)) / tm * 100, 2),
                gain_exceeds_parent_range=bool(gain > rng), loss_within_parent_range=bool(gain > -rng))


def isa(lib):
    funcs, meta = I.collect(lib)
    by_name = {I.short_name(k).replace('void ', ''): v for k, v in funcs.items()}
    regs = {I.demangle(k).replace('void ', ''): v for k, v in meta.items()}
    out = {}
    for n in sorted(k for k in by_name if k.startswith('k_closed<')):
        c, m = by_name[n], regs[n]
        out[n] = dict(instructions=c['_total'], valu=sum(c[k] for k in I.VALU_CLASSES), salu=c['salu'], lds=c['lds'], vmem=c['vmem'],
                      scratch_instructions=c['scratch'], vgpr=int(m['vgpr_count']), sgpr=int(m['sgpr_count']),
                      sgpr_spill=int(m['sgpr_spill_count']), vgpr_spill=int(m['vgpr_spill_count']),
                      scratch_bytes=int(m['private_segment_fixed_size']))
    return out


def pmc(path):
    k = json.load(open(path))['k_closed']
    return {'shape': k['shape'], 'src_hash': k['src_hash'], **{x: k[x] for x in PMC_KEYS if x in k}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('out')
    ap.add_argument('parent_lib')
    ap.add_argument('--pmc-before')
    ap.add_argument('--isa-notes')
    a = ap.parse_args()
    d = a.out
    res = {'note': 'One MI355X, tools/hidden_obs_bench.sh: every command alternated between the parent commit\'s library and this tree\'s '
                   '(D2D_LIB).  bench_* values are env-steps/s of bench.py\'s closed loop (600_300 and 20_5: config 2, 4096 envs, '
                   'k_closed<1, true>; config3 / config4 / config5: --workload); closed_65536 = tools/closed_loop_bench.py --envs 65536 '
                   '--streams 1; chain_prof = the -DD2D_CHAIN_PROF builds; kernel_trace = the k_closed dispatches of `rocprofv3 '
                   '--kernel-trace --stats` over the 600 / 300 command, a pass of its own; pmc = profiles/pmc_latest.json of the parent '
                   'commit and of this tree (tools/gpu_profile_all.sh, counters in runs of their own).',
           'runs': {}, 'summary': {}}
    for name in ('bench_600_300', 'bench_20_5', 'bench_config3', 'bench_config4', 'bench_config5', 'closed_65536'):
        p, t = runs(d, name, 'parent'), runs(d, name, 'this')
        if p and t:
            res['runs'][name] = {'parent': p, 'this': t}
            res['summary'][name] = summary(p, t)
    for which in ('parent', 'this'):
        res.setdefault('chain_prof', {})[which] = open(os.path.join(d, f'chain_prof_{which}.out')).read().splitlines()[:14]
        rows = list(csv.DictReader(open(os.path.join(d, f'kernel_trace_closed_{which}.csv'))))
        kc = [r for r in rows if 'k_closed<' in r['Kernel_Name']]
        res.setdefault('kernel_trace', {})[which] = dict(
            kernel=sorted({I.short_name(r['Kernel_Name']).replace('void ', '') for r in kc}),
            launches_us=[round((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3, 1) for r in kc],
            vgpr_count=sorted({int(r['VGPR_Count']) for r in kc}), scratch_size=sorted({int(r['Scratch_Size']) for r in kc}))
    res['summary']['kernel_trace_mean_us'] = {k: round(st.mean(v['launches_us']), 1) for k, v in res['kernel_trace'].items()}
    res['isa'] = {'parent': isa(a.parent_lib), 'this': isa(THIS)}
    if a.isa_notes:
        res['isa']['by_hand'] = json.load(open(a.isa_notes))
    if a.pmc_before:
        b, t = pmc(a.pmc_before), pmc(os.path.join(ROOT, 'profiles', 'pmc_latest.json'))
        res['pmc_per_env_step'] = {'before': b, 'after': t,
                                   'drop': {k: round(b[k] - t[k], 1) for k in PMC_KEYS if k in b and k in t}}
    json.dump(res, sys.stdout, indent=1)
    print()


if __name__ == '__main__':
    main()
